// Host side of the C ABI declared in include/synergy_hip.h: constant packing (BatchNorm -> per
// channel scale/shift, weight repack, basis repack into MFMA operand order), workspace, and the
// launch sequence of the MobileNetV2 forward (reference mobilenetv2_backbone.py:173-189).
#include "../../include/synergy_hip.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <string>
#include <vector>

#include "syn_internal.h"
#include "bcast_protocol.h"

namespace {

thread_local std::string g_err;

int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) return fail(SYN_ERR_HIP, "%s -> %s", #expr, hipGetErrorString(e_)); \
    } while (0)

struct DeviceGuard {   // torch tracks the current device per thread: never leave it changed
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

enum Kind { STEM = 0, PW = 1, DW = 2 };

struct Layer {
    Kind kind;
    int cin, cout, stride, relu6, residual;
    int hin, hout;       // spatial size in / out
    int feature;         // index into .features
    int kpad, npad;      // packed GEMM dims (PW)
    size_t src_w;        // offsets (floats) into the flat host input
    size_t dst_w, dst_scale, dst_shift;   // offsets (floats) into the packed device blob
    size_t dst_wpk;      // PW layers of fused blocks: weights in MFMA lane order (fused_block.hip)
    size_t dst_wb3;      // PW layers of features.5-17: fp16 x2 split (features.2-4: 3-way bf16 split), lane order of v_mfma_f32_16x16x32_* (dwords)
    size_t dst_scl;      // ... of features.5-17: {S, 1/S, 6 S, 0}, S = the power of two the fp16 pieces of the layer are scaled by
    size_t dst_wrm;      // PW layers of features.2-4: fragments of the row-marching kernel (fused_block_rm.hip), or 0
    size_t dst_wlb;      // project layers of features.8-13: fragments of the register-resident kernel (fused_block_lb.hip), or 0
    size_t dst_tlb;      // expand layers of features.8-13: per hidden group [12][32] floats = depthwise filter 9 rows | depthwise shift | expand shift | constants
    size_t dst_weh;      // expand layers of features.8-13: fp16 x2 fragments of the register-resident kernel, or 0
    size_t dst_glb;      // expand layers of features.15-17: per hidden group one run [We | Wp | constants] for fused_block_lb4.hip, or 0
};

int round_up(int v, int m) { return (v + m - 1) / m * m; }

// Network table: reference mobilenetv2_backbone.py:107-117 (t,c,n,s), :129-143 (features), :55 (residual).
struct Net {
    std::vector<Layer> layers;
    size_t flat_count = 0;      // floats in the host flat input (incl. heads)
    size_t src_fc = 0;
    size_t packed_count = 0;    // floats in the packed device blob
    size_t dst_fc_w = 0, dst_fc_b = 0, dst_head_f16 = 0;   // dst_head_f16: features.18 weights as 2 fp16 pieces (dwords) + their power-of-two scale
    size_t dst_range = 0;                                 // 64 dwords: {unsafe1, unsafe16 (bit masks), in_bound[20], min_wmean[20], w_relerr[20]}
    size_t max_io = 0, max_hidden = 0;   // per-face activation floats (block in/out, expanded)
    double flops = 0, pw_flops = 0;
    Net() {
        static const int cfg[7][4] = {{1, 16, 1, 1}, {6, 24, 2, 2}, {6, 32, 3, 2}, {6, 64, 4, 2},
                                      {6, 96, 3, 1}, {6, 160, 3, 2}, {6, 320, 1, 1}};
        auto add = [&](Kind k, int cin, int cout, int stride, int relu6, int residual, int hin, int feature) {
            Layer L{};
            L.kind = k; L.cin = cin; L.cout = cout; L.stride = stride; L.relu6 = relu6; L.residual = residual;
            L.hin = hin; L.hout = (stride == 2) ? (hin + 1) / 2 : hin;   // k=3,p=1,s=2: floor((h-1)/2)+1
            L.feature = feature;
            L.kpad = round_up(cin, 16); L.npad = round_up(cout, 64);
            layers.push_back(L);
        };
        add(STEM, 3, 32, 2, 1, 0, 120, 0);
        int inp = 32, h = 60, f = 1;
        for (auto &c : cfg) {
            for (int i = 0; i < c[2]; ++i) {
                const int stride = i == 0 ? c[3] : 1, hid = inp * c[0];
                const int res = (stride == 1 && inp == c[1]);
                if (c[0] != 1) add(PW, inp, hid, 1, 1, 0, h, f);
                add(DW, hid, hid, stride, 1, 0, h, f);
                h = layers.back().hout;
                add(PW, hid, c[1], 1, 0, res, h, f);
                inp = c[1];
                ++f;
            }
        }
        add(PW, 320, 1280, 1, 1, 0, h, 18);
        size_t src = 0, dst = 0;
        for (auto &L : layers) {
            size_t wn, wp;
            if (L.kind == STEM) { wn = 32 * 27; wp = 27 * 32; }
            else if (L.kind == DW) { wn = (size_t)L.cout * 9; wp = 9 * (size_t)L.cout; }
            else { wn = (size_t)L.cout * L.cin; wp = (size_t)L.npad * L.kpad; }
            const int cpad = L.kind == PW ? L.npad : L.cout;
            L.src_w = src; src += wn + 4 * (size_t)L.cout;
            L.dst_w = dst; dst += wp;
            L.dst_scale = dst; dst += cpad;
            L.dst_shift = dst; dst += cpad;
            // fused kernels: BN scale folded into the weights (accumulators start at the BN shift):
            // PW in MFMA lane order, stem [27][32] and depthwise [9][C] as plain scaled copies
            L.dst_wpk = dst;
            if (L.kind == PW) dst += (size_t)round_up(L.cout, 16) * round_up(L.cin, 16);
            else dst += wp;
            L.dst_wb3 = 0;
            L.dst_scl = 0;
            if (L.kind == PW && L.feature >= 5 && L.feature <= 17 && L.cin % 32 == 0) {
                L.dst_wb3 = dst;
                dst += (size_t)round_up(L.cout, 16) * L.cin;              // 2 fp16 per weight
                L.dst_scl = dst; dst += 4;
            }
            if (L.kind == PW && L.feature >= 2 && L.feature <= 4) {
                // early blocks: expand K (16 / 24) zero padded to one k32 step; project K = hidden chunks of
                // early_block_hc() channels, each padded to k32 steps (fused_block_early.hip)
                L.dst_wb3 = dst;
                const int hc = L.relu6 ? L.cin : syn::early_block_hc(L.cin);
                const int steps = (L.relu6 ? 1 : L.cin / hc) * (round_up(hc, 32) / 32);
                dst += (size_t)(round_up(L.cout, 16) / 16) * steps * 512;
            }
            L.dst_wrm = 0;
            if (L.kind == PW && L.feature >= 2 && L.feature <= 6) {
                L.dst_wrm = dst;
                dst += L.relu6 ? syn::rm_expand_dwords(L.cin, L.cout) : syn::rm_project_dwords(L.cin);
                if (!L.dst_scl) { L.dst_scl = dst; dst += 4; }
            }
            if (L.kind == PW && L.feature == 1) { L.dst_wrm = dst; dst += syn::rm_project_dwords(L.cin); L.dst_scl = dst; dst += 4; }     // stem_rm.hip
            L.dst_wlb = 0;
            if (L.kind == PW && !L.relu6 && L.feature >= 7 && L.feature <= 14) { L.dst_wlb = dst; dst += syn::lb_project_dwords(L.cin, L.cout); }
            L.dst_tlb = 0;
            L.dst_glb = 0;
            if (L.kind == PW && L.relu6 && L.feature >= 15 && L.feature <= 17) {
                const int cout_p = L.feature == 17 ? 320 : 160;
                L.dst_glb = dst; dst += syn::lb4_group_dwords(L.cin, cout_p) * (size_t)(L.cout / 32);
            }
            L.dst_weh = 0;
            if (L.kind == PW && L.relu6 && L.feature >= 7 && L.feature <= 14) {
                L.dst_tlb = dst; dst += syn::lb_table_floats(L.cout);
                L.dst_weh = dst; dst += syn::lb_expand_dwords(L.cin, L.cout);
            }
            if (L.kind == STEM) { L.dst_wrm = dst; dst += syn::rm_stem_dwords(); }
            if (L.kind == STEM) {            // stem filter as bf16 x3 MFMA fragments: [n_tile 2][piece 3][lane 64][4 dwords]
                L.dst_wb3 = dst;
                dst += 2 * 3 * 64 * 4;
            }
            const double pix = (double)L.hout * L.hout;
            const double f2 = L.kind == STEM ? 2.0 * 27 * 32 * pix : L.kind == DW ? 2.0 * 9 * L.cout * pix
                                                                                   : 2.0 * L.cin * (double)L.cout * pix;
            flops += f2;
            if (L.kind == PW) pw_flops += f2;
            const size_t out_sz = (size_t)L.cout * L.hout * L.hout;
            const bool hidden = (L.kind == DW) || (L.kind == PW && L.relu6);   // expand / dw outputs (and features.18)
            if (hidden) max_hidden = out_sz > max_hidden ? out_sz : max_hidden;
            else max_io = out_sz > max_io ? out_sz : max_io;
        }
        src_fc = src; src += 62 * 1280 + 62;
        flat_count = src;
        dst_fc_w = dst; dst += 64 * 1280;
        dst_fc_b = dst; dst += 64;
        dst_head_f16 = dst; dst += (size_t)80 * 10 * 2 * 256 + 4;        // fragments, then {S, 1/S}
        dst_range = dst; dst += 64;                                      // the verdict of analyze_mbv2_ranges (RangeInfo), travels with the blob
        packed_count = dst;
        flops += 2.0 * 1280 * 62;
    }
};

const Net &net() {
    static const Net n;
    return n;
}

// ---- ResNet-50 (BASELINE config 5): reference backbone_nets/resnet_backbone.py:90-136 (Bottleneck, stride on the 3x3),
// :139-254 (ResNet: 7x7/2 stem, 3x3/2 max-pool, layers [3,4,6,3], heads tex/ori/shape/exp -> cat(ori,shape,exp,tex)).
struct RConv {
    int cin, cout, k, stride, pad, hin, hout;
    size_t src_w, dst_w, dst_scale, dst_shift, dst_w3;   // dst_w3: fp16 x2 split scaled by a power of two, MFMA lane order (dwords), then {S, 1/S}
    size_t dst_wrm = 0;                                   // stem only: fragments + folded shift of resnet_stem_mfma_kernel
    size_t dst_w1f = 0;                                   // conv1 of a block that follows another block: its fragments step-major for conv_c3f_kernel (dwords), or 0
};
struct RBlock {
    int c1, c2, c3, ds;
    size_t dst_w3d = 0, dst_ones = 0, dst_shiftd = 0;   // stride-2 downsample blocks: conv3 and the branch as ONE GEMM (folded weights' fragments, ones, summed shifts), or 0
    int dual_idx = -1;                                   // bit of the third range word: the folded weights fail the fp16 weight criterion
};
struct ResNet50 {
    std::vector<RConv> convs;      // convs[0] = stem
    std::vector<RBlock> blocks;
    size_t flat_count = 0, packed_count = 0, src_fc = 0, dst_fc_w = 0, dst_fc_b = 0, dst_range = 0;
    size_t buf_big = 0, buf_mid = 0;   // per-face floats: block in/out/identity/stem, bottleneck intermediates
    double flops = 0;
    ResNet50() {
        auto add = [&](int cin, int cout, int k, int stride, int hin) {
            RConv c{};
            c.cin = cin; c.cout = cout; c.k = k; c.stride = stride; c.pad = k / 2; c.hin = hin;
            c.hout = (hin + 2 * c.pad - k) / stride + 1;
            convs.push_back(c);
            return (int)convs.size() - 1;
        };
        add(3, 64, 7, 2, 120);                       // -> 60, then max-pool -> 30
        int inpl = 64, h = 30;
        static const int planes[4] = {64, 128, 256, 512}, nblk[4] = {3, 4, 6, 3};
        std::vector<std::pair<int, int>> order;      // state_dict order of conv indices is c1,c2,c3,(ds) per block
        for (int L = 0; L < 4; ++L)
            for (int i = 0; i < nblk[L]; ++i) {
                const int stride = (i == 0 && L > 0) ? 2 : 1, w = planes[L], outc = w * 4;
                RBlock b{};
                b.c1 = add(inpl, w, 1, 1, h);
                b.c2 = add(w, w, 3, stride, h);
                const int ho = convs[b.c2].hout;
                b.c3 = add(w, outc, 1, 1, ho);
                b.ds = (i == 0) ? add(inpl, outc, 1, stride, h) : -1;     // stride != 1 or inplanes != planes*4 (:208-212)
                blocks.push_back(b);
                inpl = outc; h = ho;
            }
        size_t src = 0, dst = 0;
        std::vector<char> follows(convs.size(), 0);          // conv1 of every block but the first: fed by the previous block's conv3 (same resolution)
        for (size_t bi = 1; bi < blocks.size(); ++bi) follows[blocks[bi].c1] = 1;
        for (auto &c : convs) {
            const size_t wn = (size_t)c.cout * c.cin * c.k * c.k;
            c.src_w = src; src += wn + 4 * (size_t)c.cout;
            const int npad = round_up(c.cout, 64);
            c.dst_w = dst; dst += (size_t)npad * c.cin * c.k * c.k;
            c.dst_scale = dst; dst += npad;
            c.dst_shift = dst; dst += npad;
            c.dst_w3 = 0;
            if (c.cin % 32 == 0) { c.dst_w3 = dst; dst += (size_t)npad * c.cin * c.k * c.k + 4; }      // two fp16 per weight, then {S, 1/S}
            if (c.cin == 3) { c.dst_wrm = dst; dst += syn::rn_stem_dwords(); }
            if (follows[&c - convs.data()] && c.cin <= 512) { c.dst_w1f = dst; dst += (size_t)c.cout * c.cin; }      // (fused launches exist up to 512 input channels)
            flops += 2.0 * c.cin * c.k * c.k * (double)c.cout * c.hout * c.hout;
            const size_t osz = (size_t)c.cout * c.hout * c.hout;
            buf_big = osz > buf_big ? osz : buf_big;
        }
        {
            int nd = 0;
            for (auto &b : blocks)
                if (b.ds >= 0 && convs[b.ds].stride == 2) {
                    const RConv &c3 = convs[b.c3], &cd = convs[b.ds];
                    b.dst_w3d = dst; dst += (size_t)c3.cout * (c3.cin + cd.cin) + 4;
                    b.dst_ones = dst; dst += c3.cout;
                    b.dst_shiftd = dst; dst += c3.cout;
                    b.dual_idx = nd++;
                }
        }
        buf_mid = 128 * 30 * 30;                      // largest conv1 / conv2 output (layer2.0.conv1: 128 x 30 x 30)
        src_fc = src; src += (size_t)102 * 2048 + 102;
        flat_count = src;
        dst_fc_w = dst; dst += (size_t)104 * 2048;
        dst_fc_b = dst; dst += 104;
        dst_range = dst; dst += 4;                    // 2 dwords: bit i = the packed fp16 x2 weights of convs[i] fail the weight criterion -> fp32-MFMA conv
        packed_count = dst;
        flops += 2.0 * 2048 * 102;
    }
};
const ResNet50 &resnet50() {
    static const ResNet50 n;
    return n;
}

// ---- MobileNetV1 (reference backbone_nets/mobilenetv1_backbone.py:47-140): conv1 + bn1 + ReLU, 13 DepthWiseBlocks (:21-44), average
// pool, heads ori / shape / exp / tex concatenated in that order (:132-138).  arch ids 2 = mobilenet_1, 3 = mobilenet_05, 4 = mobilenet_2
// (include/synergy_hip.h); widths 0.25 and 0.75 give 8 / 24 channels, no multiple of the 16-wide MFMA tile, and are not offered.
constexpr int kArchMb1First = 2, kArchLast = 4;
bool is_mb1(int arch) { return arch >= kArchMb1First && arch <= kArchLast; }
// The whole id table: 0 mobilenet_v2 | 1 resnet50 | 2 mobilenet_1 | 3 mobilenet_05 | 4 mobilenet_2 | 5: never assigned | 6 ghostnet |
// 7: never assigned | 8 resnest50 | 9: never assigned | 10 resnet18 | 11 resnet34.
constexpr int kArchGhost = 6, kArchResnest = 8, kArchRes18 = 10, kArchRes34 = 11;
bool is_gn(int arch) { return arch == kArchGhost; }
bool is_rs(int arch) { return arch == kArchResnest; }
bool is_bb(int arch) { return arch == kArchRes18 || arch == kArchRes34; }      // the BasicBlock ResNets
// (arch_known, arch_name and everything else that depends on the id alone: the table of architectures behind the descriptors, arch_info)

// ---- What the four exact-fp32 families (MobileNetV1, GhostNet, ResNeSt-50, resnet18 / 34) share: how a state_dict is laid out.
// ConvBn = a convolution and the BatchNorm behind it.  flat: weight [cout][cin][k][k], then the BN's weight | bias | running_mean |
// running_var, cout each; packed: the weights in the order its packer gives them (pack_conv / pack_conv_t below), the folded scale [cout],
// the folded shift [cout].  A depthwise convolution has cin = 1, a grouped one has cin = the inputs of ONE group.
struct ConvBn { int cin = 0, cout = 0, k = 1, groups = 1; size_t src = 0, dst_w = 0, dst_scale = 0, dst_shift = 0; };
// The four heads: 102 x pool weights and 102 biases in flat, fc_tex in front of the others (tex_first) or behind them.  Packed are rows
// 0..61 = ori | shape | exp of a [64][pool] matrix and a bias [64]; src = where fc_ori starts.  The texture head is loaded, never computed.
struct Heads { int pool = 0; size_t src = 0, dst_w = 0, dst_b = 0; };
// The cursor a *Net constructor walks its table with: floats taken so far from the flat input and given so far to the packed blob, in
// the module's state_dict order, and the multiply-adds per face of what was laid out.
struct Layout {
    size_t src = 0, dst = 0;
    double macs = 0;
    size_t flat(size_t n) { const size_t at = src; src += n; return at; }         // n floats that are no ConvBn (SE vectors, fc1 / fc2, conv_head):
    size_t packed(size_t n) { const size_t at = dst; dst += n; return at; }       // where they start
    ConvBn conv(int cin, int cout, int k, int hw, int groups = 1) {                // hw = output pixels
        ConvBn c; c.cin = cin; c.cout = cout; c.k = k; c.groups = groups;
        const size_t nw = (size_t)cout * cin * k * k;
        c.src = flat(nw + 4 * (size_t)cout);
        c.dst_w = packed(nw); c.dst_scale = packed(cout); c.dst_shift = packed(cout);
        macs += (double)nw * hw;
        return c;
    }
    ConvBn depthwise(int c, int k, int hw) { return conv(1, c, k, hw); }
    ConvBn grouped3x3(int cg, int ng, int groups, int hw) { return conv(cg, groups * ng, 3, hw, groups); }
    ConvBn stem27(int c0) { return conv(3, c0, 3, 3600); }                        // 3x3 / 2 on the 120^2 crop: 27 taps
    Heads heads(int pool, bool tex_first) {                                        // (the caller counts the MACs: 62 or 102 rows, as its module does)
        Heads f; f.pool = pool;
        f.src = flat((size_t)102 * pool + 102) + (tex_first ? (size_t)40 * pool + 40 : 0);
        f.dst_w = packed((size_t)64 * pool); f.dst_b = packed(64);
        return f;
    }
};
void grow(size_t &m, size_t v) { m = v > m ? v : m; }

// ... and how the pieces of a layout are packed.  BatchNorm folds, in fp32, to y = conv * scale + shift with scale = gamma / sqrt(var + 1e-5)
// and shift = beta - mean * scale; bn = weight | bias | running_mean | running_var, c each.
void fold_bn(const float *bn, int c, float *scale, float *shift) {
    for (int i = 0; i < c; ++i) {
        const float sc = bn[i] / sqrtf(bn[3 * c + i] + 1e-5f);
        scale[i] = sc;
        shift[i] = bn[c + i] - bn[2 * c + i] * sc;
    }
}
// weight [cout][cin][k][k] -> [cout][tap][cin], as the GEMM kernels read it (a 1x1 convolution stays as it is), and the folded BN
void pack_conv(const float *flat, const ConvBn &c, std::vector<float> &pk) {
    const int kk = c.k * c.k;
    const float *w = flat + c.src;
    for (int o = 0; o < c.cout; ++o)
        for (int ci = 0; ci < c.cin; ++ci)
            for (int t = 0; t < kk; ++t) pk[c.dst_w + ((size_t)o * kk + t) * c.cin + ci] = w[((size_t)o * c.cin + ci) * kk + t];
    fold_bn(w + (size_t)c.cout * c.cin * kk, c.cout, pk.data() + c.dst_scale, pk.data() + c.dst_shift);
}
// weight [cout][cin][k][k] -> [ci * k * k + tap][cout], output channels innermost: the 27-tap stems [27][c0], the 7x7 stem [147][64] and
// every depthwise filter (cin = 1: tap-major [k * k][c]); and the folded BN
void pack_conv_t(const float *flat, const ConvBn &c, std::vector<float> &pk) {
    const int rows = c.cin * c.k * c.k;
    const float *w = flat + c.src;
    for (int o = 0; o < c.cout; ++o)
        for (int r = 0; r < rows; ++r) pk[c.dst_w + (size_t)r * c.cout + o] = w[(size_t)o * rows + r];
    fold_bn(w + (size_t)c.cout * rows, c.cout, pk.data() + c.dst_scale, pk.data() + c.dst_shift);
}
// fc_ori [12], fc_shape [40], fc_exp [10], each {weight [rows][pool], bias}, consecutive in flat -> rows 0..61 of the packed matrix and bias
void pack_heads(const float *flat, const Heads &f, std::vector<float> &pk) {
    const float *src = flat + f.src;
    static const int hn[3] = {12, 40, 10};
    int row = 0;
    for (int k = 0; k < 3; ++k) {
        memcpy(pk.data() + f.dst_w + (size_t)row * f.pool, src, sizeof(float) * hn[k] * f.pool);
        src += (size_t)hn[k] * f.pool;
        memcpy(pk.data() + f.dst_b + row, src, sizeof(float) * hn[k]);
        src += hn[k];
        row += hn[k];
    }
}

struct Mb1Block {
    int cin, cout, stride, hin, hout;
    ConvBn dw, pw;                                             // conv_dw + bn_dw, packed tap-major [9][cin]; conv_sep + bn_sep, [cout][cin]
};
struct Mb1Net {
    int c0 = 0, pool = 0;
    ConvBn stem;                                               // conv1 + bn1, packed [27][c0]
    std::vector<Mb1Block> blocks;
    Heads fc;
    size_t flat_count = 0, packed_count = 0;
    size_t buf_io = 0, buf_dw = 0;                             // per-face floats: a block's input / output, a depthwise output
    double flops = 0;
    size_t ws_per_face() const { return 2 * buf_io + buf_dw; }
    explicit Mb1Net(int num, int den) {                        // width = num / den
        auto ch = [&](int c) { return c * num / den; };        // int(c * width): exact for the three widths
        static const int tab[13][3] = {{32, 64, 1}, {64, 128, 2}, {128, 128, 1}, {128, 256, 2}, {256, 256, 1}, {256, 512, 2}, {512, 512, 1},
                                       {512, 512, 1}, {512, 512, 1}, {512, 512, 1}, {512, 512, 1}, {512, 1024, 2}, {1024, 1024, 1}};      // dw2_1 .. dw6 (:66-82)
        c0 = ch(32); pool = ch(1024);
        Layout L;
        stem = L.stem27(c0);
        buf_io = (size_t)c0 * 3600;
        int h = 60;
        for (const auto &t : tab) {
            Mb1Block b{};
            b.cin = ch(t[0]); b.cout = ch(t[1]); b.stride = t[2]; b.hin = h; b.hout = (h + 2 - 3) / b.stride + 1;      // 15 -> 8
            const int hw = b.hout * b.hout;
            b.dw = L.depthwise(b.cin, 3, hw);
            b.pw = L.conv(b.cin, b.cout, 1, hw);
            grow(buf_io, (size_t)b.cout * hw);
            grow(buf_dw, (size_t)b.cin * hw);
            blocks.push_back(b);
            h = b.hout;
        }
        fc = L.heads(pool, false);
        L.macs += 102.0 * pool;                                // the network's own count (all four heads), as syn_resnet50_flops_per_face
        flat_count = L.src;
        packed_count = L.dst;
        flops = 2.0 * L.macs;
    }
};
const Mb1Net &mb1net(int arch) {
    static const Mb1Net n1(1, 1), n05(1, 2), n2(2, 1);
    return arch == 3 ? n05 : (arch == 4 ? n2 : n1);
}

// ---- GhostNet (reference backbone_nets/ghostnet_backbone.py:76-266, width 1.0), arch id 6.  conv_stem + bn1 + ReLU, 16 GhostBottlenecks
// (blocks.0.0 .. blocks.8.3), blocks.9.0 = ConvBnAct 160 -> 960, global pool, conv_head 960 -> 1280 (bias) + ReLU, four heads.
// A GhostModule(c -> o) = primary 1x1 c -> o / 2 + BN (+ ReLU), cheap = depthwise 3x3 on primary + BN (+ ReLU), cat(primary, cheap);
// every o here is even, so the reference's [:, :oup] slice (:99) drops nothing -- GnNet() refuses a table where that is not so.
struct GnBlock {
    int cin, mid, cout, k, stride, se, hin, hout;
    bool conv_sc;
    ConvBn g1p, g2p, scp;                                      // ghost1 / ghost2 primary, shortcut 1x1: packed [cout][cin]
    ConvBn g1d, g2d, dw, scd;                                  // ghost1 / ghost2 cheap, the stride-2 conv_dw, shortcut depthwise: packed tap-major [k*k][c]
    size_t src_se, dst_rw, dst_rb, dst_ew, dst_eb;             // se.conv_reduce {weight [se][mid], bias}, se.conv_expand {weight [mid][se], bias}
};
struct GnNet {
    static constexpr int kBlocks = 16, kStem = 16, kLast = 960, kPool = 1280;
    std::vector<GnBlock> blocks;
    ConvBn stem, last;                                         // conv_stem + bn1, packed [27][16]; blocks.9.0
    Heads fc;
    size_t flat_count = 0, packed_count = 0, src_head = 0, dst_head_w = 0, dst_head_b = 0;
    // per-face floats of the workspace regions: block input / output (x 2), ghost1 output, conv_dw output, ghost2 primary, shortcut
    // depthwise and 1x1 outputs, and the small vectors (SE mean | reduced | gate; pooled 960 | 1280)
    size_t buf_io = 0, buf_g1 = 0, buf_d = 0, buf_t = 0, buf_s = 0, buf_r = 0, buf_small = 2304;
    double flops = 0;
    size_t ws_per_face() const { return 2 * buf_io + buf_g1 + buf_d + buf_t + buf_s + buf_r + buf_small; }
    GnNet() {
        static const int tab[kBlocks][6] = {      // in, mid, out, k, stride, SE reduced channels (cfgs :240-265 through _make_divisible)
            {16, 16, 16, 3, 1, 0},    {16, 48, 24, 3, 2, 0},     {24, 72, 24, 3, 1, 0},     {24, 72, 40, 5, 2, 20},
            {40, 120, 40, 5, 1, 32},  {40, 240, 80, 3, 2, 0},    {80, 200, 80, 3, 1, 0},    {80, 184, 80, 3, 1, 0},
            {80, 184, 80, 3, 1, 0},   {80, 480, 112, 3, 1, 120}, {112, 672, 112, 3, 1, 168}, {112, 672, 160, 5, 2, 168},
            {160, 960, 160, 5, 1, 0}, {160, 960, 160, 5, 1, 240}, {160, 960, 160, 5, 1, 0}, {160, 960, 160, 5, 1, 240}};
        Layout L;
        stem = L.stem27(kStem);
        buf_io = (size_t)kStem * 3600;
        int h = 60;
        for (const auto &t : tab) {
            GnBlock b{};
            b.cin = t[0]; b.mid = t[1]; b.cout = t[2]; b.k = t[3]; b.stride = t[4]; b.se = t[5];
            b.hin = h; b.hout = (h - 1) / b.stride + 1;        // pad k / 2: 60 -> 30 -> 15 -> 8 -> 4
            b.conv_sc = !(b.cin == b.cout && b.stride == 1);
            if (b.mid % 8 || b.cout % 8 || b.cin % 4 || b.se % 4) {      // halves of the concatenation must be whole float4s
                fprintf(stderr, "GnNet: block with channels %d / %d / %d / %d cannot be packed\n", b.cin, b.mid, b.cout, b.se);
                abort();
            }
            const int hw = b.hin * b.hin, hw2 = b.hout * b.hout;
            b.g1p = L.conv(b.cin, b.mid / 2, 1, hw);
            b.g1d = L.depthwise(b.mid / 2, 3, hw);
            if (b.stride == 2) b.dw = L.depthwise(b.mid, b.k, hw2);
            if (b.se) {
                const size_t wn = (size_t)b.se * b.mid;
                b.src_se = L.flat(2 * wn + b.se + b.mid);
                b.dst_rw = L.packed(wn); b.dst_rb = L.packed(b.se); b.dst_ew = L.packed(wn); b.dst_eb = L.packed(b.mid);
                L.macs += 2.0 * b.se * b.mid;
            }
            b.g2p = L.conv(b.mid, b.cout / 2, 1, hw2);
            b.g2d = L.depthwise(b.cout / 2, 3, hw2);
            if (b.conv_sc) {
                b.scd = L.depthwise(b.cin, b.k, hw2);
                b.scp = L.conv(b.cin, b.cout, 1, hw2);
            }
            grow(buf_io, (size_t)b.cout * hw2);
            grow(buf_g1, (size_t)b.mid * hw);
            grow(buf_d, (size_t)b.mid * hw2);
            grow(buf_t, (size_t)(b.cout / 2) * hw2);
            grow(buf_s, (size_t)b.cin * hw2);
            grow(buf_r, (size_t)b.cout * hw2);
            blocks.push_back(b);
            h = b.hout;
        }
        last = L.conv(160, kLast, 1, 16);
        src_head = L.flat((size_t)kPool * kLast + kPool);      // conv_head {weight [1280][960], bias}
        dst_head_w = L.packed((size_t)kPool * kLast); dst_head_b = L.packed(kPool);
        L.macs += (double)kPool * kLast;
        fc = L.heads(kPool, false);
        L.macs += 102.0 * kPool;                               // the module's own count, all four heads
        flat_count = L.src;
        packed_count = L.dst;
        flops = 2.0 * L.macs;
    }
};
const GnNet &gnnet() {
    static const GnNet n;
    return n;
}

// ---- ResNeSt-50 (reference backbone_nets/ResNeSt/resnest.py:33-41, resnet.py:29-324, splat.py:11-98), arch id 8.  Deep stem (three 3x3
// convolutions 3 -> 32 / 2, 32 -> 32, 32 -> 64), bn1 + ReLU, max pool, 3 + 4 + 6 + 3 bottlenecks of group width C = 64 / 128 / 256 / 512,
// global mean, four heads.  A bottleneck: conv1 1x1 -> C, conv2.conv 3x3 groups 2 -> 2C = U, the split-attention gate, V = att0 U0 +
// att1 U1, [3x3 / 2 average on layerN.0, N >= 2], conv3 1x1 -> 4C, + residual ([2x2 / 2 ceil-mode average], 1x1, BN on layerN.0), ReLU.
struct RsBlock {
    int cin, C, cout, inter, hin, hout;
    bool avd, down;                                            // the 3x3 / 2 average (and the 2x2 / 2 downsample pool); a downsample branch
    ConvBn c1, c3, ds;                                         // 1x1: packed [cout][cin]
    ConvBn c2;                                                 // conv2.conv, 2 groups: flat [2 C][C / 2][3][3], packed [n][9][C / 2]
    size_t src_fc = 0, dst_w1t = 0, dst_s1 = 0, dst_h1 = 0, dst_w2t = 0, dst_b2 = 0;      // flat: fc1 {weight [I][C], bias}, bn1 x4, fc2 {weight [2C][I], bias}
    // per-face floats of the block's intermediates: conv1 output, U, V, the pooled V, the pooled input, the downsample output
    size_t n_t1() const { return (size_t)hin * hin * C; }
    size_t n_u() const { return 2 * n_t1(); }
    size_t n_pa() const { return avd ? (size_t)hout * hout * C : 0; }
    size_t n_pd() const { return avd ? (size_t)hout * hout * cin : 0; }
    size_t n_r() const { return down ? (size_t)hout * hout * cout : 0; }
    size_t scratch() const { return 2 * n_t1() + n_u() + n_pa() + n_pd() + n_r() + 2 * (size_t)C; }
};
struct RsNet {
    static constexpr int kBlocks = 16, kStem = 32, kPool = 2048;
    std::vector<RsBlock> blocks;
    ConvBn stem, stem2, stem3;                                 // conv1.0, packed [27][32]; conv1.3 and conv1.6, packed [n][9][32]
    Heads fc;
    size_t flat_count = 0, packed_count = 0;
    size_t buf_io = 0, buf_scratch = 0;                        // per-face floats: block input / output (x 2), a block's intermediates
    double flops = 0;
    size_t ws_per_face() const { return 2 * buf_io + buf_scratch; }
    RsNet() {
        static const int layers[4][2] = {{64, 3}, {128, 4}, {256, 6}, {512, 3}};      // group width, blocks
        Layout L;
        stem = L.stem27(kStem);
        stem2 = L.grouped3x3(kStem, kStem, 1, 3600);
        stem3 = L.grouped3x3(kStem, 2 * kStem, 1, 3600);       // its BatchNorm is the model's bn1
        buf_io = (size_t)2 * kStem * 3600;
        buf_scratch = (size_t)2 * kStem * 3600 + 2 * (size_t)kStem * 3600;      // the stem: conv1, conv2 and conv3 outputs
        int h = 30, cin = 64;
        for (int l = 0; l < 4; ++l)
            for (int i = 0; i < layers[l][1]; ++i) {
                RsBlock b{};
                b.cin = cin; b.C = layers[l][0]; b.cout = 4 * b.C; b.inter = b.C / 2 > 32 ? b.C / 2 : 32;
                b.avd = l > 0 && i == 0; b.down = i == 0;
                b.hin = h; b.hout = b.avd ? (h + 1) / 2 : h;   // 30 -> 15 -> 8 -> 4, by both pools
                const int hw = b.hin * b.hin, hw2 = b.hout * b.hout;
                b.c1 = L.conv(b.cin, b.C, 1, hw);
                b.c2 = L.grouped3x3(b.C / 2, b.C, 2, hw);
                const size_t w1 = (size_t)b.inter * b.C, w2 = 2 * (size_t)b.C * b.inter;
                b.src_fc = L.flat(w1 + b.inter + 4 * (size_t)b.inter + w2 + 2 * (size_t)b.C);
                b.dst_w1t = L.packed(w1); b.dst_s1 = L.packed(b.inter); b.dst_h1 = L.packed(b.inter);
                b.dst_w2t = L.packed(w2); b.dst_b2 = L.packed(2 * (size_t)b.C);
                L.macs += 3.0 * b.C * b.inter;
                b.c3 = L.conv(b.C, b.cout, 1, hw2);
                if (b.down) b.ds = L.conv(b.cin, b.cout, 1, hw2);
                grow(buf_io, (size_t)b.cout * hw2);
                grow(buf_scratch, b.scratch());
                blocks.push_back(b);
                h = b.hout; cin = b.cout;
            }
        fc = L.heads(kPool, false);                            // fc_tex is in flat (a checkpoint has it) but is not packed
        L.macs += 62.0 * kPool;                                // the module's forward never calls fc_tex
        flat_count = L.src;
        packed_count = L.dst;
        flops = 2.0 * L.macs;
    }
};
const RsNet &rsnet() {
    static const RsNet n;
    return n;
}

// ---- resnet18 / resnet34 (reference backbone_nets/resnet_backbone.py:50-87 BasicBlock, :141-249 ResNet, :282-301), arch ids 10 / 11.
// Stem 7x7 / 2 3 -> 64 + BN + ReLU, max pool, [2,2,2,2] / [3,4,6,3] BasicBlocks of 64 / 128 / 256 / 512 channels on 30^2 / 15^2 / 8^2 /
// 4^2, global mean, four heads.  A BasicBlock: conv1 3x3 (stride 2 on layer2.0 / 3.0 / 4.0) + BN + ReLU, conv2 3x3 + BN, + identity (a
// 1x1 stride-2 convolution + BN of the input on those three blocks), ReLU.  One table, parametrised by the block counts, serves both.
struct BbBlock {
    int cin, C, hin, hout, stride;
    bool down;
    ConvBn c1, c2, ds;                                         // packed [cout][tap][cin]
};
struct BbNet {
    static constexpr int kPool = 512;
    std::vector<BbBlock> blocks;
    ConvBn stem;                                               // packed [147][64] (row ci*49 + ky*7 + kx), as resnet_stem_kernel reads it
    Heads fc;
    size_t flat_count = 0, packed_count = 0;
    size_t buf_io = 0, buf_stem = 0, buf_t1 = 0, buf_r = 0;    // per-face floats: block input / output (x 2), the stem's output, conv1's output, the downsample's output
    double flops = 0;
    int last() const { return (int)blocks.size() + 1; }        // the hook's block index of pool + heads
    size_t ws_per_face() const { return 2 * buf_io + buf_stem + buf_t1 + buf_r; }
    explicit BbNet(const int (&count)[4]) {
        static const int planes[4] = {64, 128, 256, 512};
        Layout L;
        stem = L.conv(3, 64, 7, 3600);
        buf_stem = (size_t)64 * 3600;
        buf_io = (size_t)64 * 900;
        int h = 30, cin = 64;
        for (int l = 0; l < 4; ++l)
            for (int i = 0; i < count[l]; ++i) {
                BbBlock b{};
                b.cin = cin; b.C = planes[l]; b.stride = (l > 0 && i == 0) ? 2 : 1; b.down = b.stride == 2;
                b.hin = h; b.hout = b.stride == 2 ? (h + 1) / 2 : h;      // 30 -> 15 -> 8 -> 4 (3x3 pad 1 stride 2, and 1x1 stride 2 alike)
                const int hw = b.hout * b.hout;
                b.c1 = L.conv(b.cin, b.C, 3, hw);
                b.c2 = L.conv(b.C, b.C, 3, hw);
                if (b.down) b.ds = L.conv(b.cin, b.C, 1, hw);
                grow(buf_io, (size_t)b.C * hw);
                grow(buf_t1, (size_t)b.C * hw);
                if (b.down) grow(buf_r, (size_t)b.C * hw);
                blocks.push_back(b);
                h = b.hout; cin = b.C;
            }
        fc = L.heads(kPool, true);                             // module order: fc_tex, fc_ori, fc_shape, fc_exp; fc_tex is in flat (a checkpoint has it) but is not packed
        L.macs += 62.0 * kPool;                                // the adapter takes the first 62 outputs: fc_tex does not run
        flat_count = L.src;
        packed_count = L.dst;
        flops = 2.0 * L.macs;
    }
};
const BbNet &bbnet(int arch) {
    static const int c18[4] = {2, 2, 2, 2}, c34[4] = {3, 4, 6, 3};
    static const BbNet n18(c18), n34(c34);
    return arch == kArchRes34 ? n34 : n18;
}

// ---- every architecture a handle can run, built once from the descriptors above; everything that depends on the arch id alone reads it ----
struct ArchInfo {
    int id;
    const char *name;
    size_t flat, packed, ws_per_face;      // floats: the host flat input, the packed device blob, the activations of one face
    int pool;                              // width of the pooled feature
    void (*pack)(int arch, const float *flat, std::vector<float> &pk);
};
const std::vector<ArchInfo> &arch_table();      // (defined behind the packers)
const ArchInfo *arch_info(int arch) {
    for (const ArchInfo &a : arch_table()) if (a.id == arch) return &a;
    return nullptr;
}
bool arch_known(int arch) { return arch_info(arch) != nullptr; }
const char *arch_name(int arch) { const ArchInfo *a = arch_info(arch); return a ? a->name : "?"; }

struct ConstHeader {   // first 256 bytes of an exported constants buffer
    uint64_t magic;
    uint32_t version, has_backbone, has_basis, n_vert, n_lmk, nvp, nlp, arch;
    uint64_t backbone_floats, basis_floats, total_bytes;
    uint8_t reserved[256 - 8 - 8 * 4 - 3 * 8];
};
static_assert(sizeof(ConstHeader) == 256, "header must be 256 bytes");
constexpr uint64_t kMagic = 0x53594e4833353558ull;   // "SYNH355X"
constexpr uint32_t kConstVersion = 6;                // bumped whenever the packed encoding changes (2: per-column basis scales, range verdict; 3: stem fragments for the (R, G, B, -) row ring; 4: clamp-form constants of the register-resident blocks; 5: ResNet-50 fragments with the output channels in pair order; 6: + folded conv3 | downsample fragments)

// verdict of the load-time range analysis of the fp16 x2 schedule (analyze_mbv2_ranges below); 64 dwords at Net::dst_range
struct RangeInfo {
    uint32_t unsafe1 = 0, unsafe16 = 0;      // bit f: .features[f] must not run an fp16 x2 kernel with input scale 1 / 16 (bit 0 = stem + features.1)
    float in_bound[20] = {};                  // max_k U_k of the input of .features[f] (f = 2..18); [0] = 1 (normalised pixels)
    float min_wmean[20] = {};                 // min over rows of the weighted mean bound (underflow side)
    float w_relerr[20] = {};                  // worst row of the weight criterion, as a multiple of its threshold (> 1 fails)
};

static_assert(sizeof(RangeInfo) <= 64 * sizeof(float), "RangeInfo must fit its slot in the backbone blob");

}  // namespace

// where the synergy MLPs' kernel-ready weights sit in syn_handle::d_syn (floats; syn_load_synergy)
struct SynOffsets {
    size_t tW[2][5], tscale[2][5], tshift[2][5];      // trunks conv1 .. conv5: [0] MLP_for, [1] MLP_rev
    size_t W6p, W6f, scale6, shift6, W7, scale7, shift7, W8, scale8, shift8, W9, scale9, shift9;
    size_t Wrev, scale_rev, shift_rev;                // MLP_rev's three heads as one [64][1024] layer
};

struct syn_handle {
    int device = 0;
    int arch = 0;                  // 0 = mobilenet_v2 (reference default), 1 = resnet50 (BASELINE config 5), 2 / 3 / 4 = mobilenet_1 / _05 / _2
    float *d_backbone = nullptr;   // packed_count floats
    float *d_basis = nullptr;      // dense tiles | landmark tiles | mean[64] | std[64]
    size_t basis_floats = 0;
    int n_vert = 0, n_lmk = 0, nvp = 0, nlp = 0;
    float *ws = nullptr;           // backbone activations (used on the stream of syn_backbone_forward*)
    size_t ws_bytes = 0;
    float *rec = nullptr;          // reconstruction records (used on the stream of syn_reconstruct*): an allocation of its
    size_t rec_bytes = 0;          // own, so that a backbone call of ANY batch size never overlaps records still in flight
    // mesh topology + render scratch (syn_load_triangles / syn_mesh_* / syn_rasterize)
    int *d_tri = nullptr, *d_adj_off = nullptr, *d_adj_tri = nullptr;
    int ntri = 0, tri_nver = 0;
    // textured meshes (syn_load_uv_map): UV pixel tables over all vertices, the kept-vertex list and a second topology slot
    // for the kept mesh with its own adjacency; topo_slot = which of the two syn_mesh_shade* / syn_rasterize read
    int *d_uv = nullptr;           // coord_u [uv_nver] | coord_v [uv_nver] | keep_ind [n_keep]
    int uv_nver = 0, n_keep = 0, uv_max[4] = {0, 0, 0, 0};      // max coord_u, coord_v over all vertices | over the kept ones
    int *k_tri = nullptr, *k_adj_off = nullptr, *k_adj_tri = nullptr;
    int k_ntri = 0;
    int topo_slot = 0;
    // texture coordinates of syn_render_texture, per topology slot (syn_load_tex_coords): [tex_nver,3] floats, then the slot's
    // tex_triangles [ntri,3] where the caller gave some (texc_own_tri); dropped when the slot's topology is replaced
    float *d_texc[2] = {nullptr, nullptr};
    int texc_nver[2] = {0, 0}, texc_own_tri[2] = {0, 0};
    int tri_max[2] = {0, 0};       // the largest vertex index of each slot's triangles
    void *rws = nullptr;           // render scratch: tri normals | min/max keys | z keys
    size_t rws_bytes = 0;
    // synergy refinement (syn_load_synergy / syn_refine_* / syn_landmarks_to_param): weights + per-call scratch, grown lazily
    float *d_syn = nullptr;
    float *d_syn_flat = nullptr;   // the unfolded flat state on the device (weight gradients, syn_update_synergy_device)
    SynOffsets syn_off = {};
    float *sws = nullptr;          // Lc | point features | conv6 face rows | conv6 face sums | global feature
    size_t sws_bytes = 0;
    // FaceBoxes detector: packed weights + per-frame scratch (syn_load_detector / syn_detect / syn_detect_batch)
    float *d_det = nullptr;
    void *dws = nullptr;
    size_t dws_bytes = 0;
    int early_rm = 2047;            // SYNERGY_HIP_EARLY_RM (bit 10: features.8-14 of batches <= 256 as ONE four-stream chain launch, fused_block_lb.hip; bit 4: the ResNet-50 7x7 stem on the matrix pipe, resnet_kernels.hip; bits 5, 6: features.5, 6): bit (f-2) set -> features.f (f = 2..4) runs the row-marching kernel; bit 3: the
                                   // uint8 stem + features.1 (stem_rm.hip)
                                   // (fused_block_rm.hip) instead of the tiled one (fused_block_early.hip, kept as a cross-check)
    float *d_range = nullptr;      // resnet50 run-time range guard: per-tensor max |x| of the last forward (kRangeSub sub-slots each) | its initial values
    uint32_t resnet_w_unsafe[3] = {0, 0, 0};   // bit i: convs[i] must run the fp32-MFMA kernel (weight criterion, set at load / import); word 2: bit j = the folded conv3 + downsample weights of dual block j fail it
    int resnet_gemm = 1;           // SYNERGY_HIP_RESNET_GEMM=0: every convolution on conv_h2s_kernel (cross-check of conv_lt_kernel; 2: its 128-pixel tiles only)
    int resnet_fuse = 4;           // SYNERGY_HIP_RESNET_FUSE=0: conv3 and the next conv1 as two launches (cross-check of conv_c3f_kernel); 1: conv3 + conv1 fused; 2: ... and layer 1's conv2 in front of them; 3: layer 2's too (three blocks: 270 / 243 / 245 -> 256 / 234 / 235 us); 4: conv3 + the stride-2 downsample branch of layer3.0 / 4.0 as one GEMM
    int resnet_fp32 = 0;           // sticky: the guard found a tensor outside the fp16 window -> exact fp32-MFMA convolutions from now on
    unsigned *guard_word = nullptr;    // page-locked host word the head kernel of a poisoned forward writes (mapped: guard_word_dev is its device
    unsigned *guard_word_dev = nullptr; // alias); read WITHOUT synchronisation at the entry of the next forward -> automatic switch to fp32-MFMA
    int guard_armed = 0;           // the last forward ran with the guard (syn_backbone_range_status reports nothing otherwise)
    int range_events = 0;          // automatic switches since the weights were loaded (syn_backbone_range_events)
    RangeInfo ri;                  // mobilenet_v2: which blocks may run the fp16 x2 kernels (set by syn_load_backbone / syn_import_constants)
    int range_guard = 1;           // SYNERGY_HIP_RANGE_GUARD=0: ignore the verdict (tests use it to show that the adversarial cases do break the unguarded schedule)
    int fusion = 2;                // SYNERGY_HIP_FUSION: 2 (default) fused blocks / chains, every GEMM on the fp16 matrix instructions with
                                   // two-piece operands; 1 fused blocks on the fp32-input MFMA only; 0 one kernel per layer
};

namespace {

size_t basis_float_count(int nvp, int nlp) {        // fp32 tiles | mean, std | column-scaled mean, std | fp16 x2 tiles (dense, landmark)
    return (size_t)(nvp + nlp) * 3 * syn::kBasisK + 256 + (size_t)((nvp + nlp) / 32) * 3 * syn::kBasisF16;
}
const float *basis_dense(const syn_handle *h) { return h->d_basis; }
const float *basis_lmk(const syn_handle *h) { return h->d_basis + (size_t)h->nvp * 3 * syn::kBasisK; }
const float *basis_mean(const syn_handle *h) { return h->d_basis + (size_t)(h->nvp + h->nlp) * 3 * syn::kBasisK; }
const float *basis_std(const syn_handle *h) { return basis_mean(h) + 64; }
const float *basis_mean_cs(const syn_handle *h) { return basis_mean(h) + 128; }     // de-whitening constants of the fp16 x2 path: entries 12..61
const float *basis_std_cs(const syn_handle *h) { return basis_mean(h) + 192; }      // x 2^-e_k (per basis column), [62] of the mean copy = 2^-e_u
const unsigned *basis_f16_dense(const syn_handle *h) { return reinterpret_cast<const unsigned *>(basis_mean(h) + 256); }
const unsigned *basis_f16_lmk(const syn_handle *h) { return basis_f16_dense(h) + (size_t)(h->nvp / 32) * 3 * syn::kBasisF16; }

// One activation workspace serves every backbone: resnet50 and mobilenet_2 need 1 152 000 floats per face, ResNeSt-50 1 123 456,
// resnet18 / 34 432 000 (the stem's 60^2 x 64 output the largest tensor), GhostNet less than half of the largest.
size_t ws_floats_per_face() {
    size_t m = 0;
    for (const ArchInfo &a : arch_table()) m = std::max(m, a.ws_per_face);
    return m;
}
// (every caller has vetted the id with arch_known or holds it in a handle, whose id is always a known one)
size_t backbone_floats(int arch) { const ArchInfo *a = arch_info(arch); return a ? a->packed : 0; }
size_t backbone_flat_floats(int arch) { const ArchInfo *a = arch_info(arch); return a ? a->flat : 0; }

// Both scratch regions only ever grow; growing synchronises the whole device first, so work in flight on another stream
// (synergynet_amd/streams.py runs the reconstruction of batch i beside the backbone of batch i+1) never loses its buffer.
int ensure_ws(syn_handle *h, int B) {
    const size_t need = ((size_t)B * ws_floats_per_face() + 1024) * sizeof(float);
    if (need <= h->ws_bytes) return SYN_OK;
    if (h->ws) { HIP_TRY(hipDeviceSynchronize()); HIP_TRY(hipFree(h->ws)); h->ws = nullptr; h->ws_bytes = 0; }
    HIP_TRY(hipMalloc((void **)&h->ws, need));
    h->ws_bytes = need;
    return SYN_OK;
}
int ensure_rec(syn_handle *h, int B) {
    const size_t need = ((size_t)B * syn::kRecFloatsPerFace + syn::kRecSlack) * sizeof(float);
    if (need <= h->rec_bytes) return SYN_OK;
    if (h->rec) { HIP_TRY(hipDeviceSynchronize()); HIP_TRY(hipFree(h->rec)); h->rec = nullptr; h->rec_bytes = 0; }
    HIP_TRY(hipMalloc((void **)&h->rec, need));
    h->rec_bytes = need;
    return SYN_OK;
}

// New weights: no range verdict, no sticky fp32 switch, the run-time guard disarmed and its word cleared, no unsafe convolutions.  A
// loader whose blob carries a verdict (resnet50's weight criterion; mobilenet_v2's on import) reads it back afterwards.
void reset_backbone_state(syn_handle *h) {
    h->ri = RangeInfo{};
    h->resnet_fp32 = 0; h->range_events = 0; h->guard_armed = 0;
    if (h->guard_word) { (void)hipDeviceSynchronize(); *(volatile unsigned *)h->guard_word = 0; }
    h->resnet_w_unsafe[0] = h->resnet_w_unsafe[1] = h->resnet_w_unsafe[2] = 0;
}
// The handle runs `arch` from now on, on the n packed floats of `packed` (host): waits for the device, replaces the allocation, uploads.
int install_backbone(syn_handle *h, int arch, const float *packed, size_t n) {
    DeviceGuard g(h->device);
    if (h->d_backbone) { HIP_TRY(hipDeviceSynchronize()); HIP_TRY(hipFree(h->d_backbone)); h->d_backbone = nullptr; }
    HIP_TRY(hipMalloc((void **)&h->d_backbone, n * sizeof(float)));
    HIP_TRY(hipMemcpy(h->d_backbone, packed, n * sizeof(float), hipMemcpyHostToDevice));
    h->arch = arch;
    reset_backbone_state(h);
    return SYN_OK;
}

// Pack one 32-vertex tile plane set in MFMA-operand lane order (see recon_kernels.hip):
// dst[(tile*3 + c) * 1664 + chunk*256 + lane*4 + s] = Wfull[c][32*tile + (lane&31)][8*chunk + 4*(lane>>5) + s]
void pack_basis_tiles(float *dst, int n_rows_valid, int n_tiles, const float *w_shp, const float *w_exp, const float *u,
                      const int64_t *rows /* nullable: row index triplets for landmarks */) {
    auto wfull = [&](int v, int c, int k) -> float {
        if (v >= n_rows_valid) return 0.f;
        const size_t row = rows ? (size_t)rows[3 * v + c] : (size_t)3 * v + c;   // flat[3j+i] = coord i of vertex j
        if (k < 40) return w_shp[row * 40 + k];
        if (k < 50) return w_exp[row * 10 + (k - 40)];
        if (k == 50) return u[row];
        return 0.f;
    };
    for (int t = 0; t < n_tiles; ++t)
        for (int c = 0; c < 3; ++c) {
            float *d = dst + ((size_t)t * 3 + c) * (syn::kBasisK * 32);
            for (int chunk = 0; chunk < 6; ++chunk)
                for (int lane = 0; lane < 64; ++lane)
                    for (int s = 0; s < 4; ++s)
                        d[chunk * 256 + lane * 4 + s] = wfull(32 * t + (lane & 31), c, 8 * chunk + 4 * (lane >> 5) + s);
            for (int lane = 0; lane < 64; ++lane)
                for (int s = 0; s < 2; ++s)
                    d[6 * 256 + lane * 2 + s] = wfull(32 * t + (lane & 31), c, 48 + 2 * (lane >> 5) + s);
        }
}

// fp32 -> fp16 bits, toward zero (what v_cvt_pkrtz_f16_f32 does to the activations), and back
static unsigned f16_rtz(float x) {
    unsigned u; memcpy(&u, &x, 4);
    const unsigned sgn = (u >> 16) & 0x8000u;
    const int e = (int)((u >> 23) & 0xff) - 127 + 15;
    unsigned m = u & 0x7fffffu;
    if (((u >> 23) & 0xff) == 0) return sgn;                    // fp32 zero / subnormal
    if (e >= 31) return sgn | 0x7bffu;                          // (never reached: operands are scaled below 2^14)
    if (e <= 0) return e < -10 ? sgn : sgn | ((m | 0x800000u) >> (14 - e));
    return sgn | ((unsigned)e << 10) | (m >> 13);
}
static float f16_value(unsigned h) {
    const int e = (h >> 10) & 31, m = h & 1023;
    const float v = e ? ldexpf(1.0f + m / 1024.0f, e - 15) : ldexpf((float)m, -24);
    return (h & 0x8000u) ? -v : v;
}

// the packers' power-of-two scale of a layer: max |w| S in [2^13, 2^14), the exponent clamped so that S, 6 S and S x shift stay far
// inside fp32 whatever the checkpoint holds (a layer that hits the clamp fails the weight criterion of analyze_mbv2_ranges)
static float pow2_scale(float mx) {
    int ex = 0;
    if (mx > 0.f && std::isfinite(mx)) { (void)frexpf(mx, &ex); ex = 14 - ex; }
    ex = ex < -100 ? -100 : (ex > 100 ? 100 : ex);
    return ldexpf(1.0f, ex);
}

// fp16 x2 layout of the same tiles for recon_f16_kernel (see syn_internal.h, launch_reconstruct_f16); column k (50 = the mean shape)
// x colscale[k], the column's own power of two
void pack_basis_tiles_f16(unsigned *dst, int n_rows_valid, int n_tiles, const float *w_shp, const float *w_exp, const float *u,
                         const int64_t *rows, const float *colscale /*[51]*/) {
    auto wfull = [&](int v, int c, int k) -> float {
        if (v >= n_rows_valid) return 0.f;
        const size_t row = rows ? (size_t)rows[3 * v + c] : (size_t)3 * v + c;
        if (k < 40) return w_shp[row * 40 + k] * colscale[k];
        if (k < 50) return w_exp[row * 10 + (k - 40)] * colscale[k];
        return u[row] * colscale[50];
    };
    auto split = [](float x, unsigned (&pc)[2]) {
        pc[0] = f16_rtz(x);
        pc[1] = f16_rtz(x - f16_value(pc[0]));
    };
    for (int t = 0; t < n_tiles; ++t)
        for (int c = 0; c < 3; ++c) {
            unsigned *d = dst + ((size_t)t * 3 + c) * syn::kBasisF16;
            for (int ks = 0; ks < 3; ++ks)
                for (int lane = 0; lane < 64; ++lane)
                    for (int dd = 0; dd < 4; ++dd) {
                        unsigned lo[2], hi[2];
                        const int k0 = 16 * ks + 8 * (lane >> 5) + 2 * dd;
                        split(wfull(32 * t + (lane & 31), c, k0), lo);
                        split(wfull(32 * t + (lane & 31), c, k0 + 1), hi);
                        for (int pc = 0; pc < 2; ++pc) d[((ks * 2 + pc) * 64 + lane) * 4 + dd] = lo[pc] | (hi[pc] << 16);
                    }
            // fourth k16 step (recon_prep_f16_kernel writes the matching alpha side): columns 48, 49 and the mean as split products,
            // [b48a b48a b48b | b49a b49a b49b | ua ub] in lane half 0, zeros in lane half 1
            for (int lane = 0; lane < 64; ++lane) {
                unsigned b8[2], b9[2], uu[2];
                split(wfull(32 * t + (lane & 31), c, 48), b8);
                split(wfull(32 * t + (lane & 31), c, 49), b9);
                split(wfull(32 * t + (lane & 31), c, 50), uu);
                unsigned *x = d + (6 * 64 + lane) * 4;
                if ((lane >> 5) == 0) {
                    x[0] = b8[0] | (b8[0] << 16); x[1] = b8[1] | (b9[0] << 16); x[2] = b9[0] | (b9[1] << 16); x[3] = uu[0] | (uu[1] << 16);
                } else {
                    x[0] = x[1] = x[2] = x[3] = 0u;
                }
            }
        }
}

int run_backbone(syn_handle *h, const float *img, const uint8_t *img8, int B, float *param, float *pool, hipStream_t s,
                 int stop_feature = -1, float *feature_out = nullptr, int prof_feature = -1,
                 unsigned long long *prof = nullptr, std::vector<hipEvent_t> *marks = nullptr,
                 std::vector<int> *mark_feature = nullptr, int start_feature = 0, const float *span_in = nullptr,
                 std::vector<int> *tags = nullptr) {
    const Net &n = net();
    int rc = ensure_ws(h, B);
    if (rc) return rc;
    float *X = h->ws;
    float *Y = X + (size_t)B * n.max_io;
    float *H1 = Y + (size_t)B * n.max_io;
    float *H2 = H1 + (size_t)B * n.max_hidden;
    const float *P = h->d_backbone;
    const size_t nl = n.layers.size();
    // load-time range verdict (analyze_mbv2_ranges): bit f set -> .features[f] must not run an fp16 x2 kernel with input scale 1 / 16
    const unsigned u1 = h->range_guard ? h->ri.unsafe1 : 0u, u16 = h->range_guard ? (h->ri.unsafe16 | h->ri.unsafe1) : 0u;
    auto any_unsafe16 = [&](int first, int last) { for (int f = first; f <= last; ++f) if ((u16 >> f) & 1u) return true; return false; };
    syn::HeadSliced head_sliced{nullptr, 0, nullptr, nullptr};     // features.17 left as hidden-slice partial sums for the tail to add (small batches)
    bool have_head_sliced = false;
    auto mark = [&](int feature) {          // profiling hook: one event after every launch (syn_mobilenet2_span: the code alone, no event)
        if (tags) { if (feature >= 0) tags->push_back(feature); return; }
        if (!marks) return;
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return;
        (void)hipEventRecord(e, s);
        marks->push_back(e);
        mark_feature->push_back(feature);
    };
    mark(-1);
    // test hook (syn_mobilenet2_span): enter at the first layer of .features[start_feature] with the caller's activations as the block input
    size_t li0 = 0;
    if (start_feature >= 2) {
        while (li0 < nl && n.layers[li0].feature != start_feature) ++li0;
        if (li0 == nl || !span_in) return SYN_ERR_INVALID;
        const Layer &L0 = n.layers[li0];
        HIP_TRY(hipMemcpyAsync(X, span_in, (size_t)B * L0.cin * L0.hin * L0.hin * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    for (size_t li = li0; li < nl; ++li) {
        const Layer &L = n.layers[li];
        const float *w = P + L.dst_w, *sc = P + L.dst_scale, *sh = P + L.dst_shift;
        // fused network head: stem conv + features.1 (dw + linear project) in one launch
        if (h->fusion && L.kind == STEM && stop_feature != 0) {
            const Layer &D = n.layers[li + 1], &Pj = n.layers[li + 2];
            const float *set32 = P + L.dst_wrm + syn::rm_stem_set_dwords();      // fp32 crops: the second constant set
            if (h->fusion >= 2 && (h->early_rm & 8) && !(u1 & 1u) &&
                (img8 ? syn::launch_stem_rm(img8, reinterpret_cast<const unsigned *>(P + L.dst_wrm), P + L.dst_wrm + 3 * 2 * 256, P + D.dst_wpk, P + D.dst_shift,
                                            reinterpret_cast<const unsigned *>(P + Pj.dst_wrm), P + Pj.dst_shift, P + Pj.dst_scl, X, B, s)
                      : syn::launch_stem_rm_f32(img, reinterpret_cast<const unsigned *>(set32), set32 + 3 * 2 * 256, P + D.dst_wpk, P + D.dst_shift,
                                                reinterpret_cast<const unsigned *>(P + Pj.dst_wrm), P + Pj.dst_shift, P + Pj.dst_scl, X, B, s))) {
                li += 2;
                mark(1);
                if (stop_feature == 1) {
                    HIP_TRY(hipMemcpyAsync(feature_out, X, (size_t)B * Pj.cout * Pj.hout * Pj.hout * sizeof(float), hipMemcpyDeviceToDevice, s));
                    return SYN_OK;
                }
                continue;
            }
            syn::launch_stem_block1(img, img8, P + L.dst_wpk, h->fusion >= 2 ? reinterpret_cast<const unsigned *>(P + L.dst_wb3) : nullptr, sc, sh, P + D.dst_wpk, P + D.dst_scale, P + D.dst_shift,
                                    P + Pj.dst_wpk, P + Pj.dst_scale, P + Pj.dst_shift, X, B, s);
            li += 2;
            mark(1);
            if (stop_feature == 1) {
                HIP_TRY(hipMemcpyAsync(feature_out, X, (size_t)B * Pj.cout * Pj.hout * Pj.hout * sizeof(float), hipMemcpyDeviceToDevice, s));
                return SYN_OK;
            }
            continue;
        }
        // features.7-14 (or 8-14, 8-13) as one chain launch (fused_block_lb.hip): every workgroup carries its faces through the blocks
        const int chain_mode = (h->fusion >= 2 && L.kind == PW && L.relu6 && (L.feature == 7 || L.feature == 8) && (h->early_rm & 128) && (h->early_rm & 512) &&
                                prof_feature < 0) ? syn::lb_chain_mode(B, (h->early_rm & 1024) != 0) : 0;
        const int chain_first = chain_mode == 3 ? 7 : 8, chain_last = chain_mode == 1 ? 13 : 14, chain_n = chain_last - chain_first + 1;
        if (chain_mode && L.feature == chain_first && !any_unsafe16(chain_first, chain_last) && (stop_feature < 0 || stop_feature >= chain_last) && li + 3 * chain_n <= nl &&
            n.max_hidden >= 2048 + 2 * (size_t)64 * 96 + 16 * 160 + 64 * 64) {
            // Workgroups run through the stages unsynchronised, so a buffer must never hold two tensor layouts at once -- a fast workgroup's
            // 96-channel store into X would land in the 64-channel rows a slower workgroup still reads.  X keeps the chain input; the
            // 64-channel 8x8 tensors (features.7-10) ping-pong in Y and one slice of H1 (chain from features.8: X and Y), the 96-channel
            // ones (features.11, 12; features.13 is not stored when features.14 follows) in two more, the 4x4x160 output in a fourth.
            syn::FusedBlockArgs ca[8];
            float *const Ha = H1 + (size_t)B * 2048, *const Hb = Ha + (size_t)B * 64 * 96, *const Hc = Hb + (size_t)B * 64 * 96,   // (the head's scratch rows stay free)
                  *const Hd = Hc + (size_t)B * 16 * 160;
            float *const bin7[8] = {X, Y, Hd, Y, Hd, Ha, Hb, Ha}, *const bout7[8] = {Y, Hd, Y, Hd, Ha, Hb, Ha, Hc};
            float *const bin8[7] = {X, Y, X, Y, Ha, Hb, Ha}, *const bout8[7] = {Y, X, Y, Ha, Hb, Ha, Hc};
            float *const *bin = chain_first == 7 ? bin7 : bin8, *const *bout = chain_first == 7 ? bout7 : bout8;
            bool ok = true;
            for (int i = 0; i < chain_n && ok; ++i) {
                const Layer &E = n.layers[li + 3 * i], &Dw = n.layers[li + 3 * i + 1], &Pr = n.layers[li + 3 * i + 2];
                ok = E.kind == PW && E.relu6 && E.feature == chain_first + i && E.dst_weh && E.dst_tlb && Pr.dst_wlb;
                if (!ok) break;
                ca[i] = syn::FusedBlockArgs{bin[i], P + E.dst_wpk, P + E.dst_scale, P + E.dst_shift, P + Dw.dst_wpk, P + Dw.dst_scale, P + Dw.dst_shift,
                                            P + Pr.dst_wpk, P + Pr.dst_scale, P + Pr.dst_shift, bout[i]};
                ca[i].Alb_e = reinterpret_cast<const unsigned *>(P + E.dst_weh);
                ca[i].Alb_p = reinterpret_cast<const unsigned *>(P + Pr.dst_wlb);
                ca[i].Tlb = P + E.dst_tlb;
            }
            if (ok && syn::launch_fused_chain_lb(ca, chain_first, chain_n, B, s)) {
                li += 3 * chain_n - 1;
                X = bout[chain_n - 1];                      // (a slice of H1 from here on)
                mark(100 * chain_first + chain_last);
                if (stop_feature == chain_last) {
                    const Layer &Lp = n.layers[li];
                    HIP_TRY(hipMemcpyAsync(feature_out, X, (size_t)B * Lp.cout * Lp.hout * Lp.hout * sizeof(float), hipMemcpyDeviceToDevice, s));
                    return SYN_OK;
                }
                continue;
            }
        }
        // features.15-17 as one chain launch (fused_block_lb4.hip); only features.17's output goes to global memory
        if (h->fusion >= 2 && L.kind == PW && L.relu6 && L.feature == 15 && L.dst_glb && !any_unsafe16(15, 17) && (h->early_rm & 256) && (h->early_rm & 512) && prof_feature < 0 &&
            (stop_feature < 0 || stop_feature >= 17) && li + 9 <= nl) {
            syn::FusedBlockArgs ca[3];
            bool ok = true;
            for (int i = 0; i < 3 && ok; ++i) {
                const Layer &E = n.layers[li + 3 * i], &Dw = n.layers[li + 3 * i + 1], &Pr = n.layers[li + 3 * i + 2];
                ok = E.kind == PW && E.relu6 && E.feature == 15 + i && E.dst_glb;
                if (!ok) break;
                ca[i] = syn::FusedBlockArgs{X, P + E.dst_wpk, P + E.dst_scale, P + E.dst_shift, P + Dw.dst_wpk, P + Dw.dst_scale, P + Dw.dst_shift,
                                            P + Pr.dst_wpk, P + Pr.dst_scale, P + Pr.dst_shift, Y};
                ca[i].Glb = reinterpret_cast<const unsigned *>(P + E.dst_glb);
            }
            if (ok && syn::launch_fused_chain_lb4(ca, B, s)) {
                li += 8;
                { float *t = X; X = Y; Y = t; }
                mark(1517);
                if (stop_feature == 17) {
                    const Layer &Lp = n.layers[li];
                    HIP_TRY(hipMemcpyAsync(feature_out, X, (size_t)B * Lp.cout * Lp.hout * Lp.hout * sizeof(float), hipMemcpyDeviceToDevice, s));
                    return SYN_OK;
                }
                continue;
            }
        }
        // fused block: expand (li) + depthwise (li+1) + project (li+2) in one launch
        if (h->fusion && L.kind == PW && L.relu6 && L.feature >= 2 && L.feature <= 17) {
            // the arguments of the block whose expand layer is n.layers[l0], reading xin and writing yout
            auto block_args = [&](int l0, float *xin, float *yout) {
                const Layer &E = n.layers[l0], &D = n.layers[l0 + 1], &Pj = n.layers[l0 + 2];
                syn::FusedBlockArgs a{xin, P + E.dst_wpk, P + E.dst_scale, P + E.dst_shift, P + D.dst_wpk, P + D.dst_scale, P + D.dst_shift,
                                      P + Pj.dst_wpk, P + Pj.dst_scale, P + Pj.dst_shift, yout};
                if (prof_feature == E.feature) a.prof = prof;
                const bool ok1 = !((u1 >> E.feature) & 1u), ok16 = !((u16 >> E.feature) & 1u);     // fp16 x2 kernels allowed at input scale 1 / 16
                if (h->fusion >= 2 && ok1 && E.dst_wb3 && Pj.dst_wb3) {
                    a.We3 = reinterpret_cast<const unsigned *>(P + E.dst_wb3);
                    a.Wp3 = reinterpret_cast<const unsigned *>(P + Pj.dst_wb3);
                }
                if (h->fusion >= 2 && E.dst_scl && Pj.dst_scl) { a.scl_e = P + E.dst_scl; a.scl_p = P + Pj.dst_scl; }
                if (h->fusion >= 2 && ok1 && E.dst_wrm && Pj.dst_wrm && ((h->early_rm >> (E.feature <= 4 ? E.feature - 2 : E.feature)) & 1)) {
                    a.Arm_e = reinterpret_cast<const unsigned *>(P + E.dst_wrm);
                    a.Arm_p = reinterpret_cast<const unsigned *>(P + Pj.dst_wrm);
                }
                if (h->fusion >= 2 && ok16 && a.We3 && Pj.dst_wlb && E.dst_tlb && (h->early_rm & 128)) {
                    a.Alb_p = reinterpret_cast<const unsigned *>(P + Pj.dst_wlb);
                    a.Alb_e = reinterpret_cast<const unsigned *>(P + E.dst_weh);
                    a.Tlb = P + E.dst_tlb;
                }
                if (h->fusion >= 2 && ok16 && E.dst_glb && (h->early_rm & 256)) a.Glb = reinterpret_cast<const unsigned *>(P + E.dst_glb);
                a.scratch = H2; a.scratch_floats = (size_t)B * n.max_hidden;       // (the per-layer schedule's second hidden buffer: free here)
                return a;
            };
            syn::FusedBlockArgs a = block_args(li, X, Y);
            // features.3 + 4 and features.5 + 6 as ONE launch each (fused_block_rm.hip: a workgroup marches its faces through both blocks)
            if ((L.feature == 3 || L.feature == 5) && (a.Arm_e || (L.feature == 5 && a.We3)) && prof_feature < 0 && (stop_feature < 0 || stop_feature >= L.feature + 1) && li + 6 <= nl &&
                n.layers[li + 3].kind == PW && n.layers[li + 3].relu6 && n.layers[li + 3].feature == L.feature + 1) {
                // Workgroups run through the two blocks unsynchronised, so a buffer must never hold two tensor LAYOUTS at once: features.6 writes the
                // rows of its own faces in features.5's input layout (safe), but features.4's 15x15x32 rows would land in the 30x30x24 input rows
                // of faces another workgroup has not read yet -- its output goes behind features.3's input inside the same region instead
                const Layer &Pb = n.layers[li + 5];
                const size_t in_a = (size_t)L.cin * L.hin * L.hin, out_b = (size_t)Pb.cout * Pb.hout * Pb.hout;
                float *const out2 = (L.feature == 3 && in_a + out_b <= n.max_io) ? X + (size_t)B * in_a : (L.feature == 5 ? X : nullptr);
                const syn::FusedBlockArgs b = block_args(li + 3, Y, out2);
                // (small batches: features.5 + 6 on the whole-image tiled kernel share a launch the same way -- one workgroup per face)
                if (out2 && ((a.Arm_e && b.Arm_e && syn::launch_fused_pair_rm(L.feature, a, b, B, s)) ||
                             (L.feature == 5 && a.We3 && b.We3 && B < 513 && syn::launch_fused_pair_f16(a, b, B, s)))) {
                    X = out2;                                   // (the rest of the region still holds any later block output: they only shrink)
                    li += 5;                                    // (two blocks: X -> Y -> out2)
                    mark(100 * L.feature + L.feature + 1);
                    if (stop_feature == L.feature + 1) {
                        const Layer &Lp = n.layers[li];
                        HIP_TRY(hipMemcpyAsync(feature_out, X, (size_t)B * Lp.cout * Lp.hout * Lp.hout * sizeof(float), hipMemcpyDeviceToDevice, s));
                        return SYN_OK;
                    }
                    continue;
                }
            }
            // features.17 of a small batch: only the hidden slices; the tail adds them while staging its input (no reduce launch).  Taken when the
            // fp16 x2 tail is what follows and nobody asked for features.17's tensor itself
            if (L.feature == 17 && a.Glb && stop_feature < 0 && prof_feature < 0 && !((u1 >> 18) & 1u) && syn::launch_lb4_sliced17_deferred(a, B, s, &head_sliced)) {
                have_head_sliced = true;
                float *t = X; X = Y; Y = t;
                li += 2;
                mark(L.feature);
                continue;
            }
            if ((a.Arm_e && syn::launch_fused_block_rm(L.feature, a, B, s)) ||
                (a.Alb_p && syn::launch_fused_block_lb(L.feature, a, B, s)) ||
                (a.Glb && syn::launch_fused_block_lb4(L.feature, a, B, s)) ||
                (a.We3 && (syn::launch_fused_block_early(L.feature, a, B, s) || syn::launch_fused_block_f16(L.feature, a, B, s))) ||
                syn::launch_fused_block(L.feature, a, B, s)) {
                float *t = X; X = Y; Y = t;
                li += 2;
                mark(L.feature);
                const Layer &Lp = n.layers[li];
                if (stop_feature >= 0 && Lp.feature == stop_feature) {
                    HIP_TRY(hipMemcpyAsync(feature_out, X, (size_t)B * Lp.cout * Lp.hout * Lp.hout * sizeof(float), hipMemcpyDeviceToDevice, s));
                    return SYN_OK;
                }
                continue;
            }
        }
        if (L.kind == STEM) {
            syn::launch_stem(img, img8, w, sc, sh, X, B, s);
        } else if (L.kind == DW) {
            // input: expanded H1, or the block input X for the t=1 block (no expand conv, :58-60)
            const bool has_expand = li > 0 && n.layers[li - 1].kind == PW && n.layers[li - 1].feature == L.feature;
            syn::launch_depthwise(has_expand ? H1 : X, w, sc, sh, H2, B, L.hin, L.hout, L.cout, L.stride, s);
        } else if (L.feature == 18 && h->fusion >= 2 && !((u1 >> 18) & 1u) && stop_feature != 18) {
            syn::launch_head_f16x2(X, reinterpret_cast<const unsigned *>(P + n.dst_head_f16), sh, P + n.dst_fc_w, P + n.dst_fc_b,
                                    param, pool, H1, B, s, have_head_sliced ? &head_sliced : nullptr);
            mark(19);
            HIP_TRY(hipGetLastError());
            return SYN_OK;
        } else if (L.feature == 18 && h->fusion && stop_feature != 18) {
            syn::launch_head(X, P + L.dst_wpk, sc, sh, P + n.dst_fc_w, P + n.dst_fc_b, param, pool, B, s);
            mark(19);
            HIP_TRY(hipGetLastError());
            return SYN_OK;
        } else if (L.feature == 18) {
            syn::launch_pointwise(X, w, sc, sh, nullptr, H1, B * L.hout * L.hout, L.cin, L.kpad, L.cout, 1, s);
        } else if (L.relu6) {   // expand
            syn::launch_pointwise(X, w, sc, sh, nullptr, H1, B * L.hout * L.hout, L.cin, L.kpad, L.cout, 1, s);
        } else {                // linear project (+ residual), then the block output becomes the next input
            syn::launch_pointwise(H2, w, sc, sh, L.residual ? X : nullptr, Y, B * L.hout * L.hout, L.cin, L.kpad, L.cout, 0, s);
            float *t = X; X = Y; Y = t;
        }
        mark(L.feature);
        // test hook (syn_debug_feature): hand back the NHWC output of .features[stop_feature]
        if (stop_feature >= 0 && L.feature == stop_feature && (li + 1 == nl || n.layers[li + 1].feature != L.feature)) {
            const float *src = L.feature == 18 ? H1 : X;
            HIP_TRY(hipMemcpyAsync(feature_out, src, (size_t)B * L.cout * L.hout * L.hout * sizeof(float), hipMemcpyDeviceToDevice, s));
            return SYN_OK;
        }
    }
    syn::launch_pool_fc(H1, P + n.dst_fc_w, P + n.dst_fc_b, param, pool, B, s);
    mark(19);
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

// slot of the range-guard array a ResNet-50 tensor reports into: 0 = the max-pool output, 1 + i = the output of convs[i]; only
// tensors that a later fp16 x2 convolution splits take part (not the downsample branches -- added in fp32 -- nor the last block's
// output, which goes to the pool)
constexpr int kResnetStat = 54;
bool resnet_stat_used(int slot) {
    const ResNet50 &n = resnet50();
    if (slot == 0) return true;
    const int ci = slot - 1;
    if (ci <= 0 || ci >= (int)n.convs.size()) return false;           // (the stem's output is seen through the max-pool)
    for (const RBlock &b : n.blocks) if (b.ds == ci) return false;
    return ci != n.blocks.back().c3;
}
constexpr size_t kRangeFloats = (size_t)64 * syn::kRangeSub * syn::kRangeStride;      // 64 tensors x sub-slots x stride (1 MiB)
float *range_slot(float *base, int t) { return base + (size_t)t * syn::kRangeSub * syn::kRangeStride; }
int ensure_range(syn_handle *h) {
    if (h->d_range) return SYN_OK;
    if (!h->guard_word) {
        HIP_TRY(hipHostMalloc((void **)&h->guard_word, 64, hipHostMallocMapped));
        h->guard_word[0] = 0;
        HIP_TRY(hipHostGetDevicePointer((void **)&h->guard_word_dev, h->guard_word, 0));
    }
    HIP_TRY(hipMalloc((void **)&h->d_range, 2 * kRangeFloats * sizeof(float)));      // live copy | initial values
    std::vector<float> init(kRangeFloats, 0.f);
    for (int t = 0; t < 64; ++t)
        if (!(t < kResnetStat && resnet_stat_used(t)))
            for (int i = 0; i < syn::kRangeSub; ++i) init[((size_t)t * syn::kRangeSub + i) * syn::kRangeStride] = 1.0f;
    HIP_TRY(hipMemcpy(h->d_range + kRangeFloats, init.data(), kRangeFloats * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->d_range, init.data(), kRangeFloats * sizeof(float), hipMemcpyHostToDevice));
    return SYN_OK;
}

// Entry and exit of a span (syn_resnet50_span): block 0 = stem + max-pool, 1..16 = the bottlenecks, 17 = pool + heads.  The forward's loop is
// entered at `first` on the caller's fp32 NHWC activations (first = 0: on the crops, as the forward) and left behind `last`; the production
// call passes no span and issues exactly the launches it always issued.
struct RSpan {
    int first = 0, last = 17;
    const float *in = nullptr;     // first >= 1: the input of block `first`, fp32 NHWC
    float *out = nullptr;          // last <= 16: the output of block `last`, fp32 NHWC (last = 17: param / pool are the outputs)
    float *aux = nullptr;          // last <= 15: conv1 of block last + 1 where the fused launch of block `last` produced it
    bool aux_written = false;
    syn::LaunchSink *sink = nullptr;
};

int run_resnet50(syn_handle *h, const float *img, const uint8_t *img8, int B, float *param, float *pool, hipStream_t s,
                 int n_out = 62, RSpan *sp = nullptr) {
    const ResNet50 &n = resnet50();
    int rc = ensure_ws(h, B);
    if (rc) return rc;
    float *A = h->ws, *X = A + (size_t)B * n.buf_big, *Y = X + (size_t)B * n.buf_big, *D = Y + (size_t)B * n.buf_big;
    float *T1 = D + (size_t)B * n.buf_big, *T2 = T1 + (size_t)B * n.buf_mid;
    const float *P = h->d_backbone;
    // ReLU activations have no static bound, so the fp16 x2 convolutions are guarded at run time: every tensor they split reports
    // its max |x| (resnet_kernels.hip range_note), the head kernel turns the results into NaN when one left [kRangeLo, kRangeHi],
    // and syn_backbone_range_status() lets the host switch the handle to the exact fp32-MFMA convolutions for good.
    // A forward that left the window poisoned its results AND wrote the handle's page-locked word (head kernel); seen here, without
    // a synchronisation, the handle runs the exact fp32-MFMA convolutions from now on -- a caller that never looks at
    // syn_backbone_range_status gets a NaN batch (more while poisoned forwards are still in flight), not NaN for ever.
    if (h->guard_word && *(volatile unsigned *)h->guard_word != 0 && h->range_guard) {
        *(volatile unsigned *)h->guard_word = 0;
        if (!h->resnet_fp32) { h->resnet_fp32 = 1; h->range_events += 1; }
    }
    const bool f16 = h->fusion >= 2 && !h->resnet_fp32;
    const bool guard = f16 && h->range_guard;
    h->guard_armed = guard;
    float *stat = nullptr;
    if (guard) {
        rc = ensure_range(h);
        if (rc) return rc;
        stat = h->d_range;
        HIP_TRY(hipMemcpyAsync(stat, stat + kRangeFloats, kRangeFloats * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    // f16: every tensor a convolution consumes travels in the PAIR format (resnet_kernels.hip) -- the max-pool output, the bottleneck
    // intermediates T1 / T2, the block outputs X / Y; fp32 stay the downsample branch D (only ever a residual) and the last block's output
    // (the pool reads it).  An fp32 handle (fusion < 2, or after a range event) keeps everything fp32.
    const int PF = f16 ? 1 : 0;
    // test knob resnet_exact_mask = bit set of convolutions forced onto the exact kernel inside an fp16 x2 forward (tools/dbg_resnet_exact.py)
    static const unsigned long long force_exact = (unsigned long long)syn::test_knob("resnet_exact_mask", 0);
    auto unsafe_w = [&](int ci) { return ((force_exact >> ci) & 1ull) || (h->range_guard && ((h->resnet_w_unsafe[ci >> 5] >> (ci & 31)) & 1u)); };
    // the guard slot of tensor t (0 = the max-pool output, 1 + i = the output of convs[i]), or NULL; `reported` keeps which slots a launch of
    // this call was handed: a span neutralises the others (below)
    unsigned long long reported = 0;
    auto slot = [&](int t) -> float * {
        if (!stat || !resnet_stat_used(t)) return nullptr;
        reported |= 1ull << t;
        return range_slot(stat, t);
    };
    auto conv = [&](int ci, const float *in, const float *res, float *out, int act, int out_pair, int res_pair) {
        const RConv &c = n.convs[ci];
        const int fmt = (PF && out_pair ? syn::kFmtOutPair : 0) | (PF && res_pair ? syn::kFmtResPair : 0);
        if (f16 && c.dst_w3 && !unsafe_w(ci)) {
            syn::launch_conv_f16x2(in, reinterpret_cast<const unsigned *>(P + c.dst_w3), P + c.dst_scale, P + c.dst_shift, res, out, B,
                                 c.hin, c.hout, c.cin, c.cout, c.k, c.k, c.stride, c.pad, act, s,
                                 slot(1 + ci), h->resnet_gemm, fmt);
            return;
        }
        // (a convolution whose WEIGHTS failed the fp16 criterion runs the exact kernel, but a later fp16 x2 convolution still takes its
        // output as pieces: it reports into its slot like the others -- left at 0 the slot read as "below the window" on every forward)
        syn::launch_conv(in, P + c.dst_w, P + c.dst_scale, P + c.dst_shift, res, out, B, c.hin, c.hout, c.cin, c.cout, c.k, c.k,
                         c.stride, c.pad, act, s, slot(1 + ci), PF, fmt);
    };
    // ---- span entry / exit (test hook; sp == nullptr in production) ----
    const int first = sp ? sp->first : 0, span_last = sp ? sp->last : 17;
    // a tensor between two blocks: [B,hw,hw,c] in the pair format inside an fp16 x2 forward (`pairs`), fp32 otherwise; the caller's side is fp32
    auto span_copy = [&](const float *src, float *dst, size_t pixels, int c, bool pairs, bool to_pairs) {
        if (!pairs) return hipMemcpyAsync(dst, src, pixels * c * sizeof(float), hipMemcpyDeviceToDevice, s);
        if (to_pairs) syn::launch_pair_from_f32(src, dst, pixels, c, s); else syn::launch_f32_from_pair(src, dst, pixels, c, s);
        return hipGetLastError();
    };
    // slots of guarded tensors that no launch of the span reported read as neutral (1.0, like the unguarded ones: slot 63 of the initial values)
    auto span_neutralise = [&]() {
        for (int t = 0; stat && sp && t < kResnetStat; ++t)
            if (resnet_stat_used(t) && !((reported >> t) & 1ull)) {
                const hipError_t e = hipMemcpyAsync(range_slot(stat, t), range_slot(stat + kRangeFloats, 63),
                                                    (size_t)syn::kRangeSub * syn::kRangeStride * sizeof(float), hipMemcpyDeviceToDevice, s);
                if (e != hipSuccess) return e;
            }
        return hipSuccess;
    };
    auto at_block = [&](int block) { if (sp && sp->sink) sp->sink->block = block; };
    const RConv &st = n.convs[0];
    at_block(first);
    // conv1+bn1+relu (:231-233): uint8 crops on the bf16 matrix pipe (batches that give every CU a workgroup), else the direct kernel
    // (the max-pool, :234, rides in the matrix-pipe stem's epilogue: the 60x60x64 tensor never exists)
    if (first >= 1) {           // the caller's activations are the input of block `first` (block 17 reads the last block's output: always fp32)
        const RConv &ci = first <= 16 ? n.convs[n.blocks[first - 1].c1] : n.convs[n.blocks.back().c3];
        const size_t pixels = first <= 16 ? (size_t)B * ci.hin * ci.hin : (size_t)B * ci.hout * ci.hout;
        HIP_TRY(span_copy(sp->in, X, pixels, first <= 16 ? ci.cin : ci.cout, PF && first <= 16, true));
    } else if (h->fusion >= 2 && img8 && B >= 128 && (h->early_rm & 16) && h->resnet_fuse &&
               syn::launch_resnet_stem_mfma(img8, reinterpret_cast<const unsigned *>(P + st.dst_wrm), P + st.dst_wrm + 2 * 10 * 2 * 256, X, B, s, 1, slot(0), PF)) {
    } else {
        if (!(h->fusion >= 2 && img8 && B >= 128 && (h->early_rm & 16) &&
              syn::launch_resnet_stem_mfma(img8, reinterpret_cast<const unsigned *>(P + st.dst_wrm), P + st.dst_wrm + 2 * 10 * 2 * 256, A, B, s)))
            syn::launch_resnet_stem(img, img8, P + st.dst_w, P + st.dst_scale, P + st.dst_shift, A, B, s);
        syn::launch_maxpool3x3s2(A, X, B, 60, 30, 64, s, slot(0), PF);                                      // maxpool (:234)
    }
    if (sp && span_last == 0) {
        HIP_TRY(span_copy(X, sp->out, (size_t)B * 900, 64, PF, false));
        HIP_TRY(span_neutralise());
        HIP_TRY(hipGetLastError());
        return SYN_OK;
    }
    // Bottleneck.forward (:114-136).  Where conv3 of a block and conv1 of the next can run as ONE launch (conv_c3f_kernel: layer 1, whose
    // convolutions are bound by memory throughput), the block output is not read back as conv1's operand and T1 already holds the next
    // block's conv1 output when its turn comes.
    bool have_t1 = false;
    for (size_t bi = first >= 1 ? first - 1 : 0; bi < n.blocks.size(); ++bi) {
        const RBlock &b = n.blocks[bi];
        const bool last = bi + 1 == n.blocks.size();
        at_block((int)bi + 1);
        if (!have_t1) conv(b.c1, X, nullptr, T1, 1, 1, 0);
        have_t1 = false;
        const float *identity = X;
        int id_pair = 1;                                   // the block input is a block output / the pooled stem: pair format in an fp16 x2 forward
        bool ds_done = b.ds < 0;
        bool c2_done = false;
        const bool c3f_ok = f16 && h->resnet_fuse && !last && n.convs[b.c3].dst_w3 && n.convs[n.blocks[last ? bi : bi + 1].c1].dst_w1f &&
                            n.convs[n.blocks[last ? bi : bi + 1].c1].hin == n.convs[b.c3].hout && !unsafe_w(b.c3) && !unsafe_w(n.blocks[last ? bi : bi + 1].c1) &&
                            syn::conv_c3f_supported(n.convs[b.c3].cin, n.convs[b.c3].cout, n.convs[n.blocks[last ? bi : bi + 1].c1].cout);
        // conv2 in front of the fused launch (64-channel bottlenecks, SYNERGY_HIP_RESNET_FUSE >= 2 = default): T2 never exists
        syn::C2Args c2a;
        const RConv &c2c = n.convs[b.c2];
        const int c2_max = h->resnet_fuse >= 3 ? 128 : 64;   // (3: layer 2's 128-channel bottlenecks too)
        const bool c2f = c3f_ok && h->resnet_fuse >= 2 && c2c.cin == c2c.cout && (c2c.cin == 64 || c2c.cin == 128) && c2c.cin <= c2_max && c2c.dst_w3 && !unsafe_w(b.c2) &&
                         (size_t)B * c2c.hin * c2c.hin * c2c.cin * 4 < (1ull << 31);
        if (c2f) {
            c2a.T1 = T1; c2a.W2 = reinterpret_cast<const unsigned *>(P + c2c.dst_w3); c2a.scale2 = P + c2c.dst_scale; c2a.shift2 = P + c2c.dst_shift;
            c2a.Hin = c2c.hin; c2a.Hout = c2c.hout; c2a.stride = c2c.stride; c2a.in_bytes = (unsigned)((size_t)B * c2c.hin * c2c.hin * c2c.cin * 4);
            c2a.stat2 = slot(1 + b.c2);
            c2_done = true;
        } else
            conv(b.c2, T1, nullptr, T2, 1, 1, 0);
        const syn::C2Args *c2p = c2f ? &c2a : nullptr;
        // (the fused launch reads T1 and writes the next block's T1: with conv2 in front they must be different buffers)
        float *T1n = c2f ? T2 : T1;
        if (c3f_ok) {
            const RConv &c3 = n.convs[b.c3], &c1n = n.convs[n.blocks[bi + 1].c1];
            {
                const float *s1 = P + c1n.dst_w3 + (size_t)(c1n.cout / 16) * (c1n.cin / 32) * 512;      // device {S, 1/S} of the next conv1's weights
                float *st3 = slot(1 + b.c3), *st1 = slot(1 + n.blocks[bi + 1].c1);
                const int M = B * c3.hout * c3.hout;
                // a stride-1 downsample branch on 64 channels (layer1.0) is evaluated inside the fused kernel: no launch, no 256-channel tensor
                if (b.ds >= 0 && n.convs[b.ds].stride == 1 && n.convs[b.ds].dst_w3 && !unsafe_w(b.ds)) {
                    const RConv &cd = n.convs[b.ds];
                    have_t1 = ds_done = syn::launch_conv_c3f_ds(T2, reinterpret_cast<const unsigned *>(P + c3.dst_w3), P + c3.dst_scale, P + c3.dst_shift, X,
                                                                reinterpret_cast<const unsigned *>(P + cd.dst_w3), P + cd.dst_scale, P + cd.dst_shift, Y,
                                                                reinterpret_cast<const unsigned *>(P + c1n.dst_w1f), s1, P + c1n.dst_scale, P + c1n.dst_shift, T1n,
                                                                M, c3.cin, cd.cin, c3.cout, c1n.cout, s, st3, st1, c2p);
                }
                if (!have_t1) {
                    if (!ds_done) { conv(b.ds, X, nullptr, D, 0, 0, 0); identity = D; id_pair = 0; ds_done = true; }
                    have_t1 = syn::launch_conv_c3f(T2, reinterpret_cast<const unsigned *>(P + c3.dst_w3), P + c3.dst_scale, P + c3.dst_shift, identity, Y,
                                                   reinterpret_cast<const unsigned *>(P + c1n.dst_w1f), s1, P + c1n.dst_scale, P + c1n.dst_shift, T1n,
                                                   M, c3.cin, c3.cout, c1n.cout, s, st3, st1, id_pair, c2p);
                }
            }
        }
        if (have_t1 && c2f) { float *t = T1; T1 = T2; T2 = t; }       // the next block's conv1 output sits in the other buffer
        if (c2_done && !have_t1) { conv(b.c2, T1, nullptr, T2, 1, 1, 0); c2_done = false; }      // (the fused launch did not take this shape after all)
        // conv3 and a stride-2 downsample branch as ONE GEMM (SYNERGY_HIP_RESNET_FUSE >= 4 = default; the pipelined GEMM only): layer3.0, layer4.0
        bool c3_done = false;
        if (!have_t1 && !ds_done && f16 && h->resnet_fuse >= 4 && b.dst_w3d && !((h->resnet_w_unsafe[2] >> b.dual_idx) & 1u && h->range_guard) &&
            !unsafe_w(b.c3) && !unsafe_w(b.ds) && syn::test_knob("lt_glds", 1) >= 1 && h->resnet_gemm == 1) {
            const RConv &c3 = n.convs[b.c3], &cd = n.convs[b.ds];
            c3_done = syn::launch_conv_dual(T2, X, reinterpret_cast<const unsigned *>(P + b.dst_w3d), P + b.dst_ones, P + b.dst_shiftd, Y, B, c3.hout, c3.cin,
                                            cd.hin, cd.stride, cd.cin, c3.cout, 1, s, slot(1 + b.c3),
                                            last ? 0 : syn::kFmtOutPair);
            if (c3_done) ds_done = true;
        }
        if (!ds_done) { conv(b.ds, X, nullptr, D, 0, 0, 0); identity = D; id_pair = 0; }
        if (!have_t1 && !c3_done) conv(b.c3, T2, identity, Y, 1, last ? 0 : 1, id_pair);      // out = relu(bn3(conv3) + identity)
        float *t = X; X = Y; Y = t;
        if (sp && span_last == (int)bi + 1) {      // leave behind block `last`: its output, and the next block's conv1 where the fused launch made it
            const RConv &c3 = n.convs[b.c3];
            HIP_TRY(span_copy(X, sp->out, (size_t)B * c3.hout * c3.hout, c3.cout, PF && !last, false));
            if (have_t1 && sp->aux) {
                const RConv &c1n = n.convs[n.blocks[bi + 1].c1];
                HIP_TRY(span_copy(T1, sp->aux, (size_t)B * c1n.hout * c1n.hout, c1n.cout, true, false));
                sp->aux_written = true;
            }
            if (!have_t1 && !last) reported &= ~(1ull << (1 + n.blocks[bi + 1].c1));      // (no fused launch: the next conv1 was not produced)
            HIP_TRY(span_neutralise());
            HIP_TRY(hipGetLastError());
            return SYN_OK;
        }
    }
    at_block(17);
    HIP_TRY(span_neutralise());
    // avgpool + heads; rows are packed (ori, shape, exp, tex) = the cat order (:242-246); the SynergyNet wrapper takes [:, :62]
    syn::launch_pool_fc_generic(X, P + n.dst_fc_w, P + n.dst_fc_b, param, pool, B, 16, 2048, n_out, n_out, s, stat, stat ? kResnetStat : 0,
                                stat ? h->guard_word_dev : nullptr);
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

// MobileNetV1 forward (MobileNet.forward, mobilenetv1_backbone.py:108-140).  Fused: one launch per block, the depthwise output never
// leaves the CU (mobilenet1_kernels.hip mb1_block_kernel); per-layer: a depthwise and a pointwise launch per block.  Schedule
// (SYNERGY_HIP_FUSION / syn_set_schedule): 2 (default) fused from kMb1FusedMinBatch faces on, per-layer below, where the fused
// launches are the slower ones; 1 fused at every batch size; 0 per-layer at every batch size, the cross-check.  Every product is
// exact fp32 in both, so there is no range verdict and no guard here.
bool mb1_fused(const syn_handle *h, int B) { return h->fusion == 1 || (h->fusion >= 2 && B >= syn::kMb1FusedMinBatch); }
// One layer of the forward, the ONLY place the MobileNetV1 launch arguments are derived from Mb1Net / Mb1Block: run_mobilenet1 walks
// layers 0..14 through it and syn_mobilenet1_layer runs one of them, so the two cannot drift apart.  layer 0 = stem (in8 or in -> out
// [B,60,60,c0]); 1..13 = block layer - 1 (in -> out; per-layer: the depthwise output goes through aux); 14 = pool + heads (in [B,4,4,pool]
// -> out = param [B,62], aux = pool, nullable).  mark(code, flops per face) is called after every launch; code: 0 = stem, 1 + 2 i = block i
// (fused, or its depthwise half), 2 + 2 i = its pointwise half, 27 = pool + heads.
template <class Mark>
void mb1_launch_layer(const Mb1Net &n, const float *P, int layer, bool fused, const float *in, const uint8_t *in8, int B, float *out,
                      float *aux, hipStream_t s, Mark &&mark) {
    if (layer == 0) {
        syn::launch_mb1_stem(in, in8, P + n.stem.dst_w, P + n.stem.dst_scale, P + n.stem.dst_shift, out, n.c0, B, s);
        mark(0, 2.0 * 27 * n.c0 * 3600);
    } else if (layer == 14) {
        // avgpool + heads (:127-138); the SynergyNet wrapper takes [:, :62] = ori | shape | exp, the first 62 rows as packed
        syn::launch_pool_fc_generic(in, P + n.fc.dst_w, P + n.fc.dst_b, out, aux, B, 16, n.pool, 62, 62, s);
        mark(27, 2.0 * n.pool * 62 + 16.0 * n.pool);
    } else {
        const int bi = layer - 1;
        const Mb1Block &b = n.blocks[bi];
        const ConvBn &d = b.dw, &p = b.pw;
        const double f_dw = 2.0 * 9 * b.cin * b.hout * b.hout, f_pw = 2.0 * b.cin * b.cout * b.hout * b.hout;
        if (fused) {
            syn::launch_mb1_block(in, P + d.dst_w, P + d.dst_scale, P + d.dst_shift, P + p.dst_w, P + p.dst_scale, P + p.dst_shift, out, B,
                                  b.hin, b.hout, b.cin, b.cout, b.stride, s);
            mark(1 + 2 * bi, f_dw + f_pw);
        } else {
            syn::launch_mb1_depthwise(in, P + d.dst_w, P + d.dst_scale, P + d.dst_shift, aux, B, b.hin, b.hout, b.cin, b.stride, s);
            mark(1 + 2 * bi, f_dw);
            syn::launch_mb1_pointwise(aux, P + p.dst_w, P + p.dst_scale, P + p.dst_shift, out, B * b.hout * b.hout, b.cin, b.cout, s);
            mark(2 + 2 * bi, f_pw);
        }
    }
}
// per-face element counts of a layer's input, output and aux (the depthwise output of a block, the pool of layer 14; 0 for the stem)
void mb1_layer_counts(const Mb1Net &n, int layer, size_t *n_in, size_t *n_out, size_t *n_aux) {
    if (layer == 0) { *n_in = (size_t)3 * 120 * 120; *n_out = (size_t)3600 * n.c0; *n_aux = 0; }
    else if (layer == 14) { *n_in = (size_t)16 * n.pool; *n_out = 62; *n_aux = n.pool; }
    else {
        const Mb1Block &b = n.blocks[layer - 1];
        *n_in = (size_t)b.hin * b.hin * b.cin; *n_out = (size_t)b.hout * b.hout * b.cout; *n_aux = (size_t)b.hout * b.hout * b.cin;
    }
}

// Profiling of the four exact-fp32 forwards (syn_backbone_profile): one event on the forward's stream after every launch, with the
// launch's code and its algorithmic FLOPs per face; entry 0 (code -1) marks the start.  A forward that is not profiled gets no LaunchMarks.
struct LaunchMarks {
    hipStream_t s;
    std::vector<hipEvent_t> events;
    std::vector<int> codes;
    std::vector<double> flops;
    explicit LaunchMarks(hipStream_t stream) : s(stream) {}
    LaunchMarks(const LaunchMarks &) = delete;
    ~LaunchMarks() { for (hipEvent_t e : events) (void)hipEventDestroy(e); }
    void operator()(int code, double fl) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return;
        (void)hipEventRecord(e, s);
        events.push_back(e);
        codes.push_back(code);
        flops.push_back(fl);
    }
};

int run_mobilenet1(syn_handle *h, const float *img, const uint8_t *img8, int B, float *param, float *pool, hipStream_t s,
                   LaunchMarks *marks = nullptr) {
    const Mb1Net &n = mb1net(h->arch);
    int rc = ensure_ws(h, B);
    if (rc) return rc;
    float *X = h->ws, *Y = X + (size_t)B * n.buf_io, *D = Y + (size_t)B * n.buf_io;
    const float *P = h->d_backbone;
    auto mark = [&](int code, double flops) { if (marks) (*marks)(code, flops); };
    mark(-1, 0.0);
    const bool fused = mb1_fused(h, B);
    mb1_launch_layer(n, P, 0, fused, img, img8, B, X, nullptr, s, mark);
    for (int layer = 1; layer <= 13; ++layer) {
        mb1_launch_layer(n, P, layer, fused, X, nullptr, B, Y, D, s, mark);
        float *t = X; X = Y; Y = t;
    }
    mb1_launch_layer(n, P, 14, fused, X, nullptr, B, param, pool, s, mark);
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

// ---- GhostNet forward (GhostNet.forward, ghostnet_backbone.py:214-233) ----
// Schedule (SYNERGY_HIP_FUSION / syn_set_schedule): 0 = one launch per layer; 1 = every GhostModule whose map is 15^2, 8^2 or 4^2 as one
// gn_ghost launch (25 of the 32 modules: blocks.3.0's ghost2 onward; the 60^2 and 30^2 modules have no fused kernel and stay per-layer);
// 2 (default) = as 1.  Both sum every output in the same order.
bool gn_fused(const syn_handle *h) { return h->fusion >= 1; }      // no batch threshold: measured faster at 1, 32, 128 and 1024 faces
struct GnWs { float *g1, *d, *t, *s, *r, *small; };           // a block's intermediates, B faces each (GnNet::buf_*)
GnWs gn_ws(const GnNet &n, float *base, int B) {
    GnWs w;
    w.g1 = base;
    w.d = w.g1 + (size_t)B * n.buf_g1;
    w.t = w.d + (size_t)B * n.buf_d;
    w.s = w.t + (size_t)B * n.buf_t;
    w.r = w.s + (size_t)B * n.buf_s;
    w.small = w.r + (size_t)B * n.buf_r;
    return w;
}
// One block of the forward, the ONLY place the GhostNet launch arguments are derived: run_ghostnet walks blocks 0..17 through it and
// syn_ghostnet_block runs one of them.  block 0..15 = bottleneck (in [B,hin,hin,cin] -> out [B,hout,hout,cout]; aux, nullable, = the SE gate
// [B,mid] of an SE block), 16 = ConvBnAct (in [B,4,4,160] -> out [B,4,4,960]), 17 = pool + conv_head + heads (in [B,4,4,960] -> out = param
// [B,62], aux, nullable, = the pooled feature [B,1280]).  mark(code, flops per face) is called after every launch; code = 100 (block + 1) +
// step: 0 ghost1 (primary, or the fused module), 1 ghost1 cheap, 2 conv_dw, 3 SE mean, 4 SE reduce, 5 SE expand, 6 shortcut depthwise,
// 7 shortcut 1x1, 8 ghost2 (primary, or fused), 9 ghost2 cheap; 1700 ConvBnAct; 1800 pool, 1801 conv_head, 1802 heads.
template <class Mark>
void gn_launch_block(const GnNet &n, const float *P, int block, bool fused, const float *in, int B, float *out, float *aux, const GnWs &w,
                     hipStream_t s, Mark &&mark) {
    auto pw = [&](const ConvBn &c, const float *A, int lda, const float *gate, int HW, float *C, int ldc, int act) {
        syn::launch_gn_pointwise(A, lda, P + c.dst_w, P + c.dst_scale, P + c.dst_shift, gate, HW, C, ldc, B * HW, c.cin, c.cout, act, s);
    };
    auto dw = [&](const ConvBn &d, const float *A, int lda, float *C, int ldc, const float *res, int ldr, float *pass_out, const float *pass_res,
                  int Hin, int Hout, int stride, int relu) {
        syn::launch_gn_depthwise(A, lda, P + d.dst_w, P + d.dst_scale, P + d.dst_shift, C, ldc, res, ldr, pass_out, pass_res, B, Hin, Hout, d.cout,
                                 d.k, stride, relu, s);
    };
    auto ghost = [&](const ConvBn &c, const ConvBn &d, const float *A, int lda, const float *gate, const float *res, int ldr, float *Y, int H,
                     int relu) {
        syn::launch_gn_ghost(A, lda, gate, P + c.dst_w, P + c.dst_scale, P + c.dst_shift, P + d.dst_w, P + d.dst_scale, P + d.dst_shift, res, ldr, Y,
                             B, H, c.cin, c.cout, relu, s);
    };
    if (block == 16) {
        pw(n.last, in, 160, nullptr, 16, out, GnNet::kLast, 1);
        mark(1700, 2.0 * 160 * GnNet::kLast * 16);
        return;
    }
    if (block == 17) {
        float *mean = w.small, *pool = aux ? aux : w.small + (size_t)B * GnNet::kLast;
        syn::launch_gn_mean(in, GnNet::kLast, mean, B, 16, GnNet::kLast, s);
        mark(1800, 16.0 * GnNet::kLast);
        syn::launch_gn_pointwise(mean, GnNet::kLast, P + n.dst_head_w, nullptr, P + n.dst_head_b, nullptr, 1, pool, GnNet::kPool, B, GnNet::kLast,
                                 GnNet::kPool, 1, s);
        mark(1801, 2.0 * GnNet::kLast * GnNet::kPool);
        // the SynergyNet wrapper takes [:, :62] = ori | shape | exp, the first 62 rows as packed; a 1-pixel "pool" passes the feature through
        syn::launch_pool_fc_generic(pool, P + n.fc.dst_w, P + n.fc.dst_b, out, nullptr, B, 1, GnNet::kPool, 62, 62, s);
        mark(1802, 2.0 * GnNet::kPool * 62);
        return;
    }
    const GnBlock &b = n.blocks[block];
    const int code = 100 * (block + 1), H = b.hin, H2 = b.hout, HW = H * H, HW2 = H2 * H2, m1 = b.mid / 2, o1 = b.cout / 2;
    const double f_g1 = 2.0 * HW * (b.cin * m1), f_g1d = 2.0 * HW * 9 * m1, f_g2 = 2.0 * HW2 * ((double)b.mid * o1), f_g2d = 2.0 * HW2 * 9 * o1;
    // ghost1: in -> g1 [B,H,H,mid], ReLU
    if (fused && syn::gn_ghost_exists(H)) {
        ghost(b.g1p, b.g1d, in, b.cin, nullptr, nullptr, 0, w.g1, H, 1);
        mark(code + 0, f_g1 + f_g1d);
    } else {
        pw(b.g1p, in, b.cin, nullptr, HW, w.g1, b.mid, 1);
        mark(code + 0, f_g1);
        dw(b.g1d, w.g1, b.mid, w.g1 + m1, b.mid, nullptr, 0, nullptr, nullptr, H, H, 1, 1);
        mark(code + 1, f_g1d);
    }
    const float *cur = w.g1;
    if (b.stride == 2) {          // conv_dw + bn_dw, no ReLU
        dw(b.dw, w.g1, b.mid, w.d, b.mid, nullptr, 0, nullptr, nullptr, H, H2, 2, 0);
        mark(code + 2, 2.0 * HW2 * b.k * b.k * b.mid);
        cur = w.d;
    }
    const float *gate = nullptr;
    if (b.se) {                   // the gate is applied where ghost2 loads its operand: the gated tensor is never stored
        float *mean = w.small, *red = mean + (size_t)B * b.mid, *gt = aux ? aux : red + (size_t)B * b.se;
        syn::launch_gn_mean(cur, b.mid, mean, B, HW2, b.mid, s);
        mark(code + 3, (double)HW2 * b.mid);
        syn::launch_gn_pointwise(mean, b.mid, P + b.dst_rw, nullptr, P + b.dst_rb, nullptr, 1, red, b.se, B, b.mid, b.se, 1, s);
        mark(code + 4, 2.0 * b.mid * b.se);
        syn::launch_gn_pointwise(red, b.se, P + b.dst_ew, nullptr, P + b.dst_eb, nullptr, 1, gt, b.mid, B, b.se, b.mid, 2, s);
        mark(code + 5, 2.0 * b.mid * b.se);
        gate = gt;
    }
    const float *res = in;
    int ldr = b.cin;
    if (b.conv_sc) {              // depthwise k x k with the block's stride + BN, 1x1 + BN, no ReLU
        dw(b.scd, in, b.cin, w.s, b.cin, nullptr, 0, nullptr, nullptr, H, H2, b.stride, 0);
        mark(code + 6, 2.0 * HW2 * b.k * b.k * b.cin);
        pw(b.scp, w.s, b.cin, nullptr, HW2, w.r, b.cout, 0);
        mark(code + 7, 2.0 * HW2 * b.cin * b.cout);
        res = w.r;
        ldr = b.cout;
    }
    // ghost2: cur (* gate) -> out [B,H2,H2,cout], no ReLU, + shortcut.  `cheap` reads `primary` WITHOUT the shortcut, so per-layer the
    // primary goes to a scratch tensor and the depthwise launch stores both halves.
    if (fused && syn::gn_ghost_exists(H2)) {
        ghost(b.g2p, b.g2d, cur, b.mid, gate, res, ldr, out, H2, 0);
        mark(code + 8, f_g2 + f_g2d);
    } else {
        pw(b.g2p, cur, b.mid, gate, HW2, w.t, o1, 0);
        mark(code + 8, f_g2);
        dw(b.g2d, w.t, o1, out + o1, b.cout, res + o1, ldr, out, res, H2, H2, 1, 0);
        mark(code + 9, f_g2d);
    }
}
int gn_launch_count(const GnNet &n, bool fused) {
    int c = 1 + 1 + 3;            // stem, ConvBnAct, pool + conv_head + heads
    for (const GnBlock &b : n.blocks)
        c += (fused && syn::gn_ghost_exists(b.hin) ? 1 : 2) + (b.stride == 2) + (b.se ? 3 : 0) + (b.conv_sc ? 2 : 0) + (fused && syn::gn_ghost_exists(b.hout) ? 1 : 2);
    return c;
}

// conv_stem + bn1 + ReLU: normalised fp32 crops NCHW [B,3,120,120] (img) or uint8 HWC crops (img8) -> [B,60,60,16].  run_ghostnet and
// block 18 of syn_ghostnet_block both launch it here.
void gn_launch_stem(const GnNet &n, const float *P, const float *img, const uint8_t *img8, int B, float *out, hipStream_t s) {
    syn::launch_mb1_stem(img, img8, P + n.stem.dst_w, P + n.stem.dst_scale, P + n.stem.dst_shift, out, GnNet::kStem, B, s);
}

int run_ghostnet(syn_handle *h, const float *img, const uint8_t *img8, int B, float *param, float *pool, hipStream_t s,
                 LaunchMarks *marks = nullptr) {
    const GnNet &n = gnnet();
    int rc = ensure_ws(h, B);
    if (rc) return rc;
    float *X = h->ws, *Y = X + (size_t)B * n.buf_io;
    const GnWs w = gn_ws(n, Y + (size_t)B * n.buf_io, B);
    const float *P = h->d_backbone;
    auto mark = [&](int code, double flops) { if (marks) (*marks)(code, flops); };
    mark(-1, 0.0);
    const bool fused = gn_fused(h);
    gn_launch_stem(n, P, img, img8, B, X, s);
    mark(0, 2.0 * 27 * GnNet::kStem * 3600);
    for (int block = 0; block <= 16; ++block) {
        gn_launch_block(n, P, block, fused, X, B, Y, nullptr, w, s, mark);
        float *t = X; X = Y; Y = t;
    }
    gn_launch_block(n, P, 17, fused, X, B, param, pool, w, s, mark);
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

// ---- ResNeSt-50 forward (ResNet.forward, ResNeSt/resnet.py:298-324) ----
// Schedule (SYNERGY_HIP_FUSION / syn_set_schedule): 0 = per-layer: V = att0 U0 + att1 U1, its 3x3 / 2 average and the downsample's
// 2x2 / 2 average are stored, one launch each, and conv3 / the downsample convolution read them; 1 = fused: conv3 (and the downsample
// convolution of layer2.0 / 3.0) build those operands once per workgroup in LDS; 2 (default) = as 1.  Both call the same device functions for the operands and the same GEMM loop: bit-identical results.
bool rs_fused(const syn_handle *h) { return h->fusion >= 1; }      // no batch threshold: measured faster at 1, 32, 128 and 1024 faces
// One block of the forward, the ONLY place the ResNeSt launch arguments are derived: run_resnest50 walks blocks 0..17 through it and
// syn_resnest50_block runs one of them.  block 0 = stem + max pool (in8 uint8 HWC crops, or in = fp32 crops, NCHW when in_hwc == 0 and
// HWC otherwise, normalised -> out [B,30,30,64]); 1..16 = the bottlenecks layer1.0 .. layer4.2 (in [B,hin,hin,cin] -> out
// [B,hout,hout,4C]; aux, nullable, = the attention [B,2C] in fc2's order); 17 = pool + heads (in [B,4,4,2048] -> out = param [B,62],
// aux, nullable, = the pool [B,2048]).  scr = B x RsNet::buf_scratch floats.  mark(code, flops per face) is called after every launch;
// code: 0 / 1 / 2 the stem convolutions, 3 the max pool; 100 block + step with step 0 conv1, 1 conv2.conv, 2 gate, 3 downsample pool,
// 4 downsample convolution, 5 combine, 6 avd pool, 7 conv3 (per-layer) or the fused tail; 1700 pool + heads.
template <class Mark>
void rs_launch_block(const RsNet &n, const float *P, int block, bool fused, const float *in, const uint8_t *in8, int in_hwc, int B,
                     float *out, float *aux, float *scr, hipStream_t s, Mark &&mark) {
    auto gemm = [&](int op, const ConvBn &c, const float *A, const float *att, const float *res, float *Y, int Hin, int Ho, int relu) {
        syn::launch_rs_gemm(op, A, c.cin, att, P + c.dst_w, P + c.dst_scale, P + c.dst_shift, res, Y, B, Hin, Ho, c.cin, c.cout, relu, s);
    };
    auto conv3 = [&](const ConvBn &c, const float *X, float *Y, int H) {      // c.cin inputs and c.cout / c.groups outputs per group
        syn::launch_rs_conv3x3(X, c.cin * c.groups, P + c.dst_w, P + c.dst_scale, P + c.dst_shift, Y, B, H, c.cin, c.cout / c.groups, c.groups, s);
    };
    if (block == 0) {
        float *s1 = scr, *s2 = s1 + (size_t)B * 3600 * RsNet::kStem, *s3 = s2 + (size_t)B * 3600 * RsNet::kStem;
        syn::launch_rs_stem(in, in8, in_hwc, P + n.stem.dst_w, P + n.stem.dst_scale, P + n.stem.dst_shift, s1, B, s);
        mark(0, 2.0 * 27 * RsNet::kStem * 3600);
        conv3(n.stem2, s1, s2, 60);
        mark(1, 2.0 * 9 * RsNet::kStem * RsNet::kStem * 3600);
        conv3(n.stem3, s2, s3, 60);
        mark(2, 2.0 * 9 * RsNet::kStem * 2 * RsNet::kStem * 3600);
        syn::launch_maxpool3x3s2(s3, out, B, 60, 30, 2 * RsNet::kStem, s);
        mark(3, 0.0);
        return;
    }
    if (block == 17) {
        // global mean + heads (:309-320); the SynergyNet wrapper's 62 = ori | shape | exp, the rows as packed
        syn::launch_pool_fc_generic(in, P + n.fc.dst_w, P + n.fc.dst_b, out, aux, B, 16, RsNet::kPool, 62, 62, s);
        mark(1700, 2.0 * RsNet::kPool * 62);
        return;
    }
    const RsBlock &b = n.blocks[block - 1];
    const int code = 100 * block, H = b.hin, H2 = b.hout, HW = H * H, HW2 = H2 * H2;
    float *t1 = scr, *u = t1 + B * b.n_t1(), *v = u + B * b.n_u(), *pa = v + B * b.n_t1(), *pd = pa + B * b.n_pa(), *r = pd + B * b.n_pd();
    float *att = aux ? aux : r + B * b.n_r();
    gemm(syn::kRsPlain, b.c1, in, nullptr, nullptr, t1, H, H, 1);
    mark(code + 0, 2.0 * HW * b.cin * b.C);
    conv3(b.c2, t1, u, H);
    mark(code + 1, 2.0 * HW * 9 * (b.C / 2) * 2 * b.C);
    syn::launch_rs_gate(u, P + b.dst_w1t, P + b.dst_s1, P + b.dst_h1, P + b.dst_w2t, P + b.dst_b2, att, B, HW, b.C, b.inter, s);
    mark(code + 2, 2.0 * 3 * b.C * b.inter);
    const float *res = in;
    if (b.down) {
        const double f_ds = 2.0 * HW2 * b.cin * b.cout;
        if (b.avd && fused && syn::rs_tail_exists(b.cin, b.cout)) gemm(syn::kRsDsPool, b.ds, in, nullptr, nullptr, r, H, H2, 0);
        else if (b.avd) {
            syn::launch_rs_dspool(in, pd, B, H, H2, b.cin, s);
            mark(code + 3, 0.0);
            gemm(syn::kRsPlain, b.ds, pd, nullptr, nullptr, r, H2, H2, 0);
        } else gemm(syn::kRsPlain, b.ds, in, nullptr, nullptr, r, H, H2, 0);      // layer1.0: AvgPool2d(1, 1) is the identity
        mark(code + 4, f_ds);
        res = r;
    }
    const double f_c3 = 2.0 * HW2 * b.C * b.cout;
    if (fused) gemm(b.avd ? syn::kRsAvd : syn::kRsCombine, b.c3, u, att, res, out, H, H2, 1);
    else {
        syn::launch_rs_combine(u, att, v, B, HW, b.C, s);
        mark(code + 5, 0.0);
        const float *a = v;
        if (b.avd) {
            syn::launch_rs_avd(v, pa, B, H, H2, b.C, s);
            mark(code + 6, 0.0);
            a = pa;
        }
        gemm(syn::kRsPlain, b.c3, a, nullptr, res, out, H2, H2, 1);
    }
    mark(code + 7, f_c3);
}
int rs_launch_count(const RsNet &n, bool fused) {
    int c = 4 + 1;                // the stem's three convolutions and the max pool; pool + heads
    for (const RsBlock &b : n.blocks)
        c += (fused ? 4 : 5) + (b.down ? 1 : 0) + (b.avd && !fused ? 1 : 0) + (b.avd && !(fused && syn::rs_tail_exists(b.cin, b.cout)) ? 1 : 0);
    return c;                     // 74 fused (layer4.0's downsample pool, K = 1024, stays a launch of its own), 95 per layer
}
// per-face element counts of a hook block's input, output and aux
void rs_block_counts(const RsNet &n, int block, size_t *n_in, size_t *n_out, size_t *n_aux) {
    if (block == 0) { *n_in = (size_t)3 * 120 * 120; *n_out = (size_t)900 * 64; *n_aux = 0; }
    else if (block == 17) { *n_in = (size_t)16 * RsNet::kPool; *n_out = 62; *n_aux = RsNet::kPool; }
    else {
        const RsBlock &b = n.blocks[block - 1];
        *n_in = (size_t)b.hin * b.hin * b.cin; *n_out = (size_t)b.hout * b.hout * b.cout; *n_aux = 2 * (size_t)b.C;
    }
}

int run_resnest50(syn_handle *h, const float *img, const uint8_t *img8, int B, float *param, float *pool, hipStream_t s,
                  LaunchMarks *marks = nullptr) {
    const RsNet &n = rsnet();
    int rc = ensure_ws(h, B);
    if (rc) return rc;
    float *X = h->ws, *Y = X + (size_t)B * n.buf_io, *scr = Y + (size_t)B * n.buf_io;
    const float *P = h->d_backbone;
    auto mark = [&](int code, double flops) { if (marks) (*marks)(code, flops); };
    mark(-1, 0.0);
    const bool fused = rs_fused(h);
    rs_launch_block(n, P, 0, fused, img, img8, 0, B, X, nullptr, scr, s, mark);
    for (int block = 1; block <= 16; ++block) {
        rs_launch_block(n, P, block, fused, X, nullptr, 0, B, Y, nullptr, scr, s, mark);
        float *t = X; X = Y; Y = t;
    }
    rs_launch_block(n, P, 17, fused, X, nullptr, 0, B, param, pool, scr, s, mark);
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

// ---- resnet18 / resnet34 forward (ResNet._forward_impl, resnet_backbone.py:227-249) ----
// Schedule (SYNERGY_HIP_FUSION / syn_set_schedule): 0 = per-layer: every 3x3 convolution reads its taps from global memory
// (bb_conv3x3_kernel), the downsample of layer2.0 / 3.0 / 4.0 is a launch of its own; 1 = LDS-tiled: bb_conv3x3_lds_kernel, conv1 of those
// three blocks also produces the downsample; 2 (default) = as 1.  Every output is the same MFMA sequence in both: bit-identical results.
bool bb_fused(const syn_handle *h) { return h->fusion >= 1; }      // no batch threshold: measured faster at 1, 32, 128 and 1024 faces
// One block of the forward, the ONLY place the launch arguments are derived: run_resnet_basic walks blocks 0 .. last through it and
// syn_resnet_basic_block runs one of them.  block 0 = stem + max pool (in8 uint8 HWC crops, or in = normalised fp32 NCHW crops -> out
// [B,30,30,64]); 1 .. last - 1 = the BasicBlocks (in [B,hin,hin,cin] -> out [B,hout,hout,C]); last = pool + heads (in [B,4,4,512] -> out =
// param [B,62], pool, nullable, [B,512]).  scr = B x (buf_stem + buf_t1 + buf_r) floats.  mark(code, flops per face) is called after every
// launch; code: 0 the stem, 1 the max pool; 100 block + step with step 0 conv1 (with the downsample when fused), 1 the downsample,
// 2 conv2; 100 last pool + heads.
template <class Mark>
void bb_launch_block(const BbNet &n, const float *P, int block, bool fused, const float *in, const uint8_t *in8, int B, float *out,
                     float *pool, float *scr, hipStream_t s, Mark &&mark) {
    if (block == 0) {
        syn::launch_resnet_stem(in, in8, P + n.stem.dst_w, P + n.stem.dst_scale, P + n.stem.dst_shift, scr, B, s);
        mark(0, 2.0 * 147 * 64 * 3600);
        syn::launch_maxpool3x3s2(scr, out, B, 60, 30, 64, s);
        mark(1, 0.0);
        return;
    }
    if (block == n.last()) {
        syn::launch_pool_fc_generic(in, P + n.fc.dst_w, P + n.fc.dst_b, out, pool, B, 16, BbNet::kPool, 62, 62, s);
        mark(100 * block, 2.0 * BbNet::kPool * 62);
        return;
    }
    const BbBlock &b = n.blocks[block - 1];
    const int code = 100 * block, H = b.hin, H2 = b.hout;
    float *t1 = scr + (size_t)B * n.buf_stem, *r = t1 + (size_t)B * n.buf_t1;
    const double f1 = 2.0 * 9 * b.cin * b.C * H2 * H2, f2 = 2.0 * 9 * b.C * b.C * H2 * H2, fd = 2.0 * b.cin * b.C * H2 * H2;
    auto conv = [&](const ConvBn &c, const ConvBn *ds, const float *X, const float *res, float *Y, int hin, int stride) {
        const float *w = P + c.dst_w, *sc = P + c.dst_scale, *sh = P + c.dst_shift;
        if (!fused) syn::launch_bb_conv3x3(X, w, sc, sh, res, Y, B, hin, H2, c.cin, c.cout, stride, 1, s);
        else syn::launch_bb_conv3x3_lds(X, w, sc, sh, res, Y, ds ? P + ds->dst_w : nullptr, ds ? P + ds->dst_scale : nullptr,
                                        ds ? P + ds->dst_shift : nullptr, ds ? r : nullptr, B, hin, H2, c.cin, c.cout, stride, 1, s);
    };
    conv(b.c1, b.down ? &b.ds : nullptr, in, nullptr, t1, H, b.stride);
    mark(code + 0, f1 + (b.down && fused ? fd : 0.0));
    if (b.down && !fused) {
        syn::launch_bb_down1x1(in, P + b.ds.dst_w, P + b.ds.dst_scale, P + b.ds.dst_shift, r, B, H, H2, b.cin, b.C, s);
        mark(code + 1, fd);
    }
    conv(b.c2, nullptr, t1, b.down ? r : in, out, H2, 1);
    mark(code + 2, f2);
}
int bb_launch_count(const BbNet &n, bool fused) {
    int c = 2 + 1;                // the stem and the max pool; pool + heads
    for (const BbBlock &b : n.blocks) c += 2 + (b.down && !fused ? 1 : 0);
    return c;                     // resnet18: 22 per layer, 19 LDS-tiled; resnet34: 38, 35
}
// per-face element counts of a hook block's input and output
void bb_block_counts(const BbNet &n, int block, size_t *n_in, size_t *n_out) {
    if (block == 0) { *n_in = (size_t)3 * 120 * 120; *n_out = (size_t)900 * 64; }
    else if (block == n.last()) { *n_in = (size_t)16 * BbNet::kPool; *n_out = 62; }
    else {
        const BbBlock &b = n.blocks[block - 1];
        *n_in = (size_t)b.hin * b.hin * b.cin; *n_out = (size_t)b.hout * b.hout * b.C;
    }
}

int run_resnet_basic(syn_handle *h, const float *img, const uint8_t *img8, int B, float *param, float *pool, hipStream_t s,
                     LaunchMarks *marks = nullptr) {
    const BbNet &n = bbnet(h->arch);
    int rc = ensure_ws(h, B);
    if (rc) return rc;
    float *X = h->ws, *Y = X + (size_t)B * n.buf_io, *scr = Y + (size_t)B * n.buf_io;
    const float *P = h->d_backbone;
    auto mark = [&](int code, double flops) { if (marks) (*marks)(code, flops); };
    mark(-1, 0.0);
    const bool fused = bb_fused(h);
    bb_launch_block(n, P, 0, fused, img, img8, B, X, nullptr, scr, s, mark);
    for (int block = 1; block < n.last(); ++block) {
        bb_launch_block(n, P, block, fused, X, nullptr, B, Y, nullptr, scr, s, mark);
        float *t = X; X = Y; Y = t;
    }
    bb_launch_block(n, P, n.last(), fused, X, nullptr, B, param, pool, scr, s, mark);
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

// what the four layer / block hooks ask of B and fused alike: the kernels index pixels (up to 3600 B) and pixel x channel quads in 32-bit integers
int check_hook_batch(const char *who, int B, int fused) {
    if (B < 1 || B > 65536) return fail(SYN_ERR_INVALID, "%s: B=%d, expected 1 <= B <= 65536", who, B);
    if (fused != 0 && fused != 1) return fail(SYN_ERR_INVALID, "%s: fused=%d, expected 0 or 1", who, fused);
    return SYN_OK;
}

}  // namespace

namespace syn {
namespace {
struct KnobTable {
    std::vector<std::pair<std::string, long long>> kv;
    KnobTable() {
        const char *e = getenv("SYNERGY_HIP_TEST_KNOBS");
        if (!e) return;
        std::string str(e);
        size_t pos = 0;
        while (pos < str.size()) {
            size_t end = str.find(',', pos);
            if (end == std::string::npos) end = str.size();
            const std::string item = str.substr(pos, end - pos);
            const size_t eq = item.find('=');
            if (eq != std::string::npos && eq > 0) kv.emplace_back(item.substr(0, eq), strtoll(item.c_str() + eq + 1, nullptr, 0));
            else if (!item.empty()) fprintf(stderr, "SYNERGY_HIP_TEST_KNOBS: ignoring '%s' (expected name=value)\n", item.c_str());
            pos = end + 1;
        }
    }
};
const KnobTable &knobs() { static const KnobTable t; return t; }
}  // namespace
long long test_knob(const char *name, long long dflt) {
    for (const auto &p : knobs().kv) if (p.first == name) return p.second;
    return dflt;
}
bool test_knob_set(const char *name) {
    for (const auto &p : knobs().kv) if (p.first == name) return true;
    return false;
}
}  // namespace syn

extern "C" {

const char *syn_last_error(void) { return g_err.c_str(); }
int syn_abi_version(void) { return 1; }

int syn_create(int device, syn_handle **out) {
    if (!out) return fail(SYN_ERR_INVALID, "syn_create: out is NULL");
    int count = 0;
    HIP_TRY(hipGetDeviceCount(&count));
    if (device < 0 || device >= count) return fail(SYN_ERR_INVALID, "syn_create: device %d of %d", device, count);
    syn_handle *h = new syn_handle();
    h->device = device;
    if (const char *e = getenv("SYNERGY_HIP_FUSION")) h->fusion = atoi(e);
    if (const char *e = getenv("SYNERGY_HIP_EARLY_RM")) h->early_rm = atoi(e);
    if (const char *e = getenv("SYNERGY_HIP_RANGE_GUARD")) h->range_guard = atoi(e);
    if (const char *e = getenv("SYNERGY_HIP_RESNET_FUSE")) h->resnet_fuse = atoi(e);
    if (const char *e = getenv("SYNERGY_HIP_RESNET_GEMM")) h->resnet_gemm = atoi(e);
    *out = h;
    return SYN_OK;
}

int syn_destroy(syn_handle *h) {
    if (h && h->d_range) { DeviceGuard g(h->device); (void)hipFree(h->d_range); h->d_range = nullptr; }
    if (h && h->guard_word) { DeviceGuard g(h->device); (void)hipDeviceSynchronize(); (void)hipHostFree(h->guard_word); h->guard_word = h->guard_word_dev = nullptr; }
    if (!h) return SYN_OK;
    DeviceGuard g(h->device);
    if (h->d_backbone) (void)hipFree(h->d_backbone);
    if (h->d_basis) (void)hipFree(h->d_basis);
    if (h->ws) (void)hipFree(h->ws);
    if (h->rec) (void)hipFree(h->rec);
    if (h->d_tri) (void)hipFree(h->d_tri);
    if (h->d_adj_off) (void)hipFree(h->d_adj_off);
    if (h->d_adj_tri) (void)hipFree(h->d_adj_tri);
    if (h->d_uv) (void)hipFree(h->d_uv);
    if (h->k_tri) (void)hipFree(h->k_tri);
    if (h->k_adj_off) (void)hipFree(h->k_adj_off);
    if (h->k_adj_tri) (void)hipFree(h->k_adj_tri);
    for (float *p : h->d_texc) if (p) (void)hipFree(p);
    if (h->rws) (void)hipFree(h->rws);
    if (h->d_syn) (void)hipFree(h->d_syn);
    if (h->d_syn_flat) (void)hipFree(h->d_syn_flat);
    if (h->sws) (void)hipFree(h->sws);
    if (h->d_det) (void)hipFree(h->d_det);
    if (h->dws) (void)hipFree(h->dws);
    delete h;
    return SYN_OK;
}

size_t syn_backbone_flat_count(void) { return net().flat_count; }
double syn_backbone_flops_per_face(void) { return net().flops; }
double syn_pointwise_flops_per_face(void) { return net().pw_flops; }
int syn_backbone_launch_count(syn_handle *h) {
    if (h && is_bb(h->arch)) return bb_launch_count(bbnet(h->arch), bb_fused(h));      // resnet18 19 / 22, resnet34 35 / 38
    if (h && is_rs(h->arch)) return rs_launch_count(rsnet(), rs_fused(h));      // 74 with the fused tail, 95 per layer
    if (h && is_gn(h->arch)) return gn_launch_count(gnnet(), gn_fused(h));      // 79 with the fused modules, 104 per layer
    if (h && is_mb1(h->arch)) return h->fusion >= 1 ? 15 : 28;      // stem + 13 blocks (x 2 per-layer) + pool and heads; schedule 2 below kMb1FusedMinBatch faces: 28
    return (int)net().layers.size() + 1;
}

// Host-only packing of the MobileNetV2 state (BN folding, MFMA lane order, bf16 x3 split): shared by syn_load_backbone and
// syn_pack_constants_host, so a blob packed without a device is byte-identical to what a handle exports.

// ---------------------------------------------------------------------------------------------------------------------------
// Load-time range analysis of the fp16 x2 schedule (csrc/*: every GEMM operand is carried as two fp16 pieces).
// fp16 has a 5-bit exponent: an operand above 65504 saturates silently in v_cvt_pkrtz_f16_f32, one below 2^-14 loses its low
// piece.  The weights are scaled per layer by the packer; the ACTIVATIONS that are split at run time are the block inputs (the
// linear, unbounded project outputs and their residual sums) at a fixed scale s: 1 in the row-marching / tiled / head kernels, 16 in
// the register-resident 8x8 / 4x4 kernels (fused_block_lb.hip, fused_block_lb4.hip).  From the folded constants alone:
//   * interval arithmetic per channel: hidden activations are in [0, 6] after ReLU6 (tighter where weights and shift say so), a
//     project output n is in shift_n + [sum_k min(w_nk lo_k, w_nk hi_k), sum_k max(...)], the residual stream adds intervals;
//   * OVERFLOW (a proof): a block may run an fp16 x2 kernel with input scale s only if s max_k U_k <= 6e4, U_k = max(|lo_k|, |hi_k|);
//   * UNDERFLOW (an estimate; the bound U may exceed the true activations by the usual slack of interval arithmetic, taken as <= 2^8):
//     the split of x_k errs by at most max(2^-20 |x_k|, 2^-24 / s); row n of the consuming GEMM keeps >= 14 bits if its weighted
//     mean bound  (sum_k |w_nk| U_k + |shift_n|) / sum_k |w_nk|  is >= 1 / (4 s);
//   * WEIGHTS (exact: the packed pieces are re-read): row n of a layer passes if sum_k |w_nk S - (a_nk + b_nk)| <=
//     2^-17 (sum_k |w_nk| S + |shift_n| S / X), X = the bound of the layer's input -- rows far below the layer's largest lose
//     their low piece to fp16 subnormals.
// A block that fails at s = 16 but passes at s = 1 runs the tiled fp16 x2 kernel (fused_block_f16.hip); one that fails at s = 1
// runs the exact fp32-MFMA kernel (fused_block.hip / stem_block1.hip / head_kernel.hip: the SYNERGY_HIP_FUSION=1 schedule).
// The verdict travels with the constants (ConstHeader) and is reported by syn_numerics_report().
// ---------------------------------------------------------------------------------------------------------------------------
struct Itv { float lo, hi; };

static void analyze_mbv2_ranges(const float *flat, RangeInfo &ri) {
    const Net &n = net();
    auto bn = [&](const Layer &L, std::vector<float> &sc, std::vector<float> &sh) {
        const size_t wn = L.kind == STEM ? 32 * 27 : L.kind == DW ? (size_t)L.cout * 9 : (size_t)L.cout * L.cin;
        const float *gamma = flat + L.src_w + wn, *beta = gamma + L.cout, *mean = beta + L.cout, *var = mean + L.cout;
        sc.resize(L.cout); sh.resize(L.cout);
        for (int c = 0; c < L.cout; ++c) { sc[c] = gamma[c] * (1.0f / sqrtf(var[c] + 1e-5f)); sh[c] = beta[c] - mean[c] * sc[c]; }
    };
    auto clip6 = [](Itv v) { return Itv{fminf(fmaxf(v.lo, 0.f), 6.f), fminf(fmaxf(v.hi, 0.f), 6.f)}; };
    // y_n = shift_n + sum_k w_nk x_k (w already BN-folded), x_k in in[k]
    auto gemm_itv = [&](const float *w, const std::vector<float> &sc, const std::vector<float> &sh, int N, int K, const std::vector<Itv> &in,
                        std::vector<Itv> &out) {
        out.resize(N);
        for (int nn = 0; nn < N; ++nn) {
            double lo = sh[nn], hi = sh[nn];
            for (int k = 0; k < K; ++k) {
                const double ww = (double)w[(size_t)nn * K + k] * sc[nn], a = ww * in[k].lo, b = ww * in[k].hi;
                lo += a < b ? a : b; hi += a < b ? b : a;
            }
            out[nn] = Itv{(float)lo, (float)hi};
        }
    };
    // depthwise 3x3 with zero padding: a tap sees its channel's interval or the padding zero
    auto dw_itv = [&](const float *w, const std::vector<float> &sc, const std::vector<float> &sh, int C, const std::vector<Itv> &in, std::vector<Itv> &out) {
        out.resize(C);
        for (int c = 0; c < C; ++c) {
            const double l = fminf(in[c].lo, 0.f), u = fmaxf(in[c].hi, 0.f);
            double lo = sh[c], hi = sh[c];
            for (int t = 0; t < 9; ++t) {
                const double ww = (double)w[(size_t)c * 9 + t] * sc[c], a = ww * l, b = ww * u;
                lo += a < b ? a : b; hi += a < b ? b : a;
            }
            out[c] = Itv{(float)lo, (float)hi};
        }
    };
    auto umax = [](const std::vector<Itv> &v) { float m = 0.f; for (const Itv &i : v) m = fmaxf(m, fmaxf(fabsf(i.lo), fabsf(i.hi))); return m; };
    // the packer's scale of a layer (the same arithmetic as pack_backbone_mbv2) and the weight criterion on the pieces it produces
    auto weight_check = [&](const float *w, const std::vector<float> &sc, const std::vector<float> &sh, int N, int K, float pre, float xbound) {
        float mx = 0.f;
        for (int nn = 0; nn < N; ++nn)
            for (int k = 0; k < K; ++k) mx = fmaxf(mx, fabsf(w[(size_t)nn * K + k] * sc[nn] * pre));
        int ex = 0;
        if (mx > 0.f) { (void)frexpf(mx, &ex); ex = 14 - ex; }
        if (!std::isfinite(mx) || ex > 100 || ex < -100) return 1e30f;          // S (or 6 S, S x shift) leaves fp32's comfortable range
        const float S = ldexpf(1.0f, ex);
        float worst = 0.f;
        for (int nn = 0; nn < N; ++nn) {
            double err = 0, mag = 0;
            for (int k = 0; k < K; ++k) {
                const float x = w[(size_t)nn * K + k] * sc[nn] * pre * S;
                const unsigned a = f16_rtz(x);
                const unsigned b = f16_rtz(x - f16_value(a));
                err += fabs((double)x - (double)f16_value(a) - (double)f16_value(b));
                mag += fabs((double)x);
            }
            mag += fabs((double)sh[nn]) * S / (xbound > 0.f ? xbound : 1.f);
            if (mag > 0) worst = fmaxf(worst, (float)(err / (mag * 7.62939453125e-6)));      // 2^-17
        }
        return worst;
    };
    auto wmean_check = [&](const float *w, const std::vector<float> &sc, const std::vector<float> &sh, int N, int K, const std::vector<Itv> &in) {
        float worst = 3.0e38f;
        for (int nn = 0; nn < N; ++nn) {
            double sw = 0, swu = 0;
            for (int k = 0; k < K; ++k) {
                const double aw = fabs((double)w[(size_t)nn * K + k] * sc[nn]);
                sw += aw; swu += aw * fmaxf(fabsf(in[k].lo), fabsf(in[k].hi));
            }
            if (sw > 0) worst = fminf(worst, (float)((swu + fabs((double)sh[nn])) / sw));
        }
        return worst;
    };
    std::vector<float> sc, sh;
    std::vector<Itv> x, e, d, y;
    const size_t nl = n.layers.size();
    auto verdict = [&](int f, float ubound, float wmean, float werr) {
        ri.in_bound[f] = ubound; ri.min_wmean[f] = wmean; ri.w_relerr[f] = fmaxf(ri.w_relerr[f], werr);
        const bool bad_w = !(werr <= 1.0f);
        if (bad_w || !(ubound <= 6.0e4f) || !(wmean >= 0.25f)) ri.unsafe1 |= 1u << f;
        if (bad_w || !(16.0f * ubound <= 6.0e4f) || !(16.0f * wmean >= 0.25f)) ri.unsafe16 |= 1u << f;
    };
    for (size_t li = 0; li < nl; ++li) {
        const Layer &L = n.layers[li];
        const float *w = flat + L.src_w;
        if (L.kind == STEM) {            // pixels (p - 127.5) / 128 in [-255/256, 255/256]; stem + features.1 = one kernel
            bn(L, sc, sh);
            std::vector<Itv> px(27, Itv{-255.0f / 256.0f, 255.0f / 256.0f});
            gemm_itv(w, sc, sh, 32, 27, px, e);
            for (Itv &v : e) v = clip6(v);
            float werr = weight_check(w, sc, sh, 32, 27, 1.0f / 128.0f, 255.0f);      // stem_rm.hip: filter / 128 against raw bytes
            werr = fmaxf(werr, weight_check(w, sc, sh, 32, 27, 1.0f, 1.0f));          // ... and its fp32-crop instantiation: the plain filter against [-1, 1]
            const Layer &D = n.layers[li + 1], &P = n.layers[li + 2];
            std::vector<float> dsc, dsh;
            bn(D, dsc, dsh);
            dw_itv(flat + D.src_w, dsc, dsh, D.cout, e, d);
            for (Itv &v : d) v = clip6(v);
            bn(P, sc, sh);
            gemm_itv(flat + P.src_w, sc, sh, P.cout, P.cin, d, x);
            werr = fmaxf(werr, weight_check(flat + P.src_w, sc, sh, P.cout, P.cin, 1.0f, 6.0f));
            ri.in_bound[0] = 1.0f; ri.min_wmean[0] = 1.0f; ri.w_relerr[0] = werr;
            if (!(werr <= 1.0f)) { ri.unsafe1 |= 1u; ri.unsafe16 |= 1u; }
            li += 2;
            continue;
        }
        if (L.kind == PW && L.relu6 && L.feature >= 2 && L.feature <= 17) {       // inverted-residual block: expand (li), dw, project
            const Layer &D = n.layers[li + 1], &P = n.layers[li + 2];
            const int f = L.feature;
            bn(L, sc, sh);
            const float ub = umax(x);
            const float wm = wmean_check(w, sc, sh, L.cout, L.cin, x);
            float werr = weight_check(w, sc, sh, L.cout, L.cin, 1.0f, ub);
            gemm_itv(w, sc, sh, L.cout, L.cin, x, e);
            for (Itv &v : e) v = clip6(v);
            std::vector<float> dsc, dsh;
            bn(D, dsc, dsh);
            dw_itv(flat + D.src_w, dsc, dsh, D.cout, e, d);
            for (Itv &v : d) v = clip6(v);
            bn(P, sc, sh);
            gemm_itv(flat + P.src_w, sc, sh, P.cout, P.cin, d, y);
            werr = fmaxf(werr, weight_check(flat + P.src_w, sc, sh, P.cout, P.cin, 1.0f, 6.0f));
            if (P.residual) for (int c = 0; c < P.cout; ++c) { y[c].lo += x[c].lo; y[c].hi += x[c].hi; }
            verdict(f, ub, wm, werr);
            x.swap(y);
            li += 2;
            continue;
        }
        if (L.kind == PW && L.feature == 18) {                                      // features.18 + pool + heads (head_kernel.hip), s = 1
            bn(L, sc, sh);
            verdict(18, umax(x), wmean_check(w, sc, sh, L.cout, L.cin, x), weight_check(w, sc, sh, L.cout, L.cin, 1.0f, umax(x)));
        }
    }
}

static void pack_backbone_mbv2(const float *flat, std::vector<float> &pk) {
    const Net &n = net();
    pk.assign(n.packed_count, 0.f);
    {
        RangeInfo ri;
        analyze_mbv2_ranges(flat, ri);
        memcpy(pk.data() + n.dst_range, &ri, sizeof ri);
    }
    for (const Layer &L : n.layers) {
        const float *w = flat + L.src_w;
        size_t wn = L.kind == STEM ? 32 * 27 : L.kind == DW ? (size_t)L.cout * 9 : (size_t)L.cout * L.cin;
        const float *gamma = w + wn, *beta = gamma + L.cout, *mean = beta + L.cout, *var = mean + L.cout;
        float *dw = pk.data() + L.dst_w;
        if (L.kind == STEM) {            // [32][3][3][3] -> [ci*9+ky*3+kx][32]
            for (int co = 0; co < 32; ++co)
                for (int t = 0; t < 27; ++t) dw[t * 32 + co] = w[co * 27 + t];
        } else if (L.kind == DW) {       // [C][1][3][3] -> [tap][C]
            for (int c = 0; c < L.cout; ++c)
                for (int t = 0; t < 9; ++t) dw[(size_t)t * L.cout + c] = w[(size_t)c * 9 + t];
        } else {                         // [N][K] -> zero padded [Npad][Kpad]
            for (int nn = 0; nn < L.cout; ++nn)
                memcpy(dw + (size_t)nn * L.kpad, w + (size_t)nn * L.cin, sizeof(float) * L.cin);
        }
        // eval-mode BatchNorm (eps 1e-5): y = x*scale + shift, the form torch's CPU kernel uses
        std::vector<float> bn_scale(L.cout);
        for (int c = 0; c < L.cout; ++c) bn_scale[c] = gamma[c] * (1.0f / sqrtf(var[c] + 1e-5f));
        if (L.kind != PW) {              // scaled copies of the stem / depthwise filters for the fused kernels
            float *dp = pk.data() + L.dst_wpk;
            const size_t taps = L.kind == STEM ? 27 : 9;
            for (size_t t = 0; t < taps; ++t)
                for (int c = 0; c < L.cout; ++c) dp[t * L.cout + c] = dw[t * L.cout + c] * bn_scale[c];
        } else {                         // [N][K] -> Wpk[n_tile][k_chunk][lane][4] (MFMA operand lane order), scale folded in
            float *dp = pk.data() + L.dst_wpk;
            const int ntl = round_up(L.cout, 16) / 16, kch = round_up(L.cin, 16) / 16;
            for (int nt = 0; nt < ntl; ++nt)
                for (int kc = 0; kc < kch; ++kc)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int q = 0; q < 4; ++q) {
                            // a trailing half chunk (cin % 16 == 8: the CIN = 24 expand layers) is walked in 2 MFMA steps:
                            // lane group g holds k = 16*kc + 2g + {0,1}, slots 2,3 unused (fused_block.hip, KHALF)
                            const bool half = (L.cin % 16 == 8) && kc == kch - 1;
                            const int nn = nt * 16 + (lane & 15);
                            const int kk = half ? (q < 2 ? kc * 16 + 2 * (lane >> 4) + q : L.cin) : kc * 16 + 4 * (lane >> 4) + q;
                            dp[(((size_t)nt * kch + kc) * 64 + lane) * 4 + q] =
                                (nn < L.cout && kk < L.cin) ? w[(size_t)nn * L.cin + kk] * bn_scale[nn] : 0.f;
                        }
        }
        if (L.dst_wb3 && L.kind == STEM) {   // K = 27 (ci*9 + ky*3 + kx) padded to one k32 chunk; lane (r16, g): k = 8g + e
            unsigned *dp = reinterpret_cast<unsigned *>(pk.data() + L.dst_wb3);
            for (int nt = 0; nt < 2; ++nt)
                for (int lane = 0; lane < 64; ++lane)
                    for (int d = 0; d < 4; ++d) {
                        unsigned pc[2][3] = {{0, 0, 0}, {0, 0, 0}};
                        const int co = nt * 16 + (lane & 15);
                        for (int e = 0; e < 2; ++e) {
                            const int k = 8 * (lane >> 4) + 2 * d + e;
                            float x = k < 27 ? w[co * 27 + k] * bn_scale[co] : 0.f;
                            for (int i = 0; i < 3; ++i) {
                                unsigned u; memcpy(&u, &x, 4); u &= 0xffff0000u;
                                float hf; memcpy(&hf, &u, 4);
                                pc[e][i] = u >> 16; x -= hf;
                            }
                        }
                        for (int i = 0; i < 3; ++i) dp[((size_t)(nt * 3 + i) * 64 + lane) * 4 + d] = pc[0][i] | (pc[1][i] << 16);
                    }
        } else if (L.dst_wb3) {          // [N][K] -> [n_tile][k32 chunk][piece][lane][4 dwords], BN scale folded in
            unsigned *dp = reinterpret_cast<unsigned *>(pk.data() + L.dst_wb3);
            auto split = [](float x, unsigned (&pc)[3]) {
                for (int i = 0; i < 3; ++i) {
                    unsigned u; memcpy(&u, &x, 4); u &= 0xffff0000u;
                    float hf; memcpy(&hf, &u, 4);
                    pc[i] = u >> 16; x -= hf;
                }
            };
            // K is walked as `nch` chunks of `hc` real channels, each zero padded to `hcp` (a multiple of 32):
            // late blocks hc = hcp = cin; early expand hc = cin (16 / 24), hcp = 32; early project hc = early_block_hc
            const bool early = L.feature >= 2 && L.feature <= 4;
            if (!early) {            // late blocks: two fp16 pieces per weight, scaled by S = 2^e to max |w| in [2^13, 2^14) (fused_block_f16.hip)
                float mx = 0.f;
                for (int nn = 0; nn < L.cout; ++nn)
                    for (int k = 0; k < L.cin; ++k) mx = fmaxf(mx, fabsf(w[(size_t)nn * L.cin + k] * bn_scale[nn]));
                                const float S = pow2_scale(mx);
                pk[L.dst_scl] = S; pk[L.dst_scl + 1] = 1.0f / S; pk[L.dst_scl + 2] = 6.0f * S;
                const int ntl = round_up(L.cout, 16) / 16, kch = L.cin / 32;
                for (int nt = 0; nt < ntl; ++nt)
                    for (int st = 0; st < kch; ++st)
                        for (int lane = 0; lane < 64; ++lane)
                            for (int d = 0; d < 4; ++d) {
                                const int nn = nt * 16 + (lane & 15), kk = 32 * st + 8 * (lane >> 4) + 2 * d;
                                float x[2] = {0.f, 0.f};
                                if (nn < L.cout) for (int e = 0; e < 2; ++e) x[e] = w[(size_t)nn * L.cin + kk + e] * bn_scale[nn] * S;
                                const unsigned a0 = f16_rtz(x[0]), a1 = f16_rtz(x[1]);
                                const unsigned b0 = f16_rtz(x[0] - f16_value(a0)), b1 = f16_rtz(x[1] - f16_value(a1));
                                dp[(((size_t)(nt * kch + st) * 2 + 0) * 64 + lane) * 4 + d] = a0 | (a1 << 16);
                                dp[(((size_t)(nt * kch + st) * 2 + 1) * 64 + lane) * 4 + d] = b0 | (b1 << 16);
                            }
            } else {                 // early blocks (fused_block_early.hip): the same two fp16 pieces and scale, their own K chunking
            // K is walked as `nch` chunks of `hc` real channels, each zero padded to `hcp` (a multiple of 32): expand hc = cin (16 / 24),
            // hcp = 32; project hc = early_block_hc
            const int hc = L.relu6 ? L.cin : syn::early_block_hc(L.cin);
            const int hcp = round_up(hc, 32), nch = L.cin / hc, spc = hcp / 32;     // k32 steps per chunk
            const int ntl = round_up(L.cout, 16) / 16, kch = nch * spc;
            float mx = 0.f;
            for (int nn = 0; nn < L.cout; ++nn)
                for (int k = 0; k < L.cin; ++k) mx = fmaxf(mx, fabsf(w[(size_t)nn * L.cin + k] * bn_scale[nn]));
                        const float S = pow2_scale(mx);                      // (= the scale the row-marching fragments of this layer use: dst_scl)
            auto put2 = [&](size_t frag, int lane, int d, float x0, float x1) {
                const unsigned a0 = f16_rtz(x0 * S), a1 = f16_rtz(x1 * S);
                const unsigned b0 = f16_rtz(x0 * S - f16_value(a0)), b1 = f16_rtz(x1 * S - f16_value(a1));
                dp[((frag * 2 + 0) * 64 + lane) * 4 + d] = a0 | (a1 << 16);
                dp[((frag * 2 + 1) * 64 + lane) * 4 + d] = b0 | (b1 << 16);
            };
            if (L.relu6 && L.cin == 16) {
                // features.2 expand: K = 16 is one step of v_mfma_f32_32x32x16_f16 -> [cout/32][piece][lane][4 dwords],
                // lane (i = l&31 channel of the 32-tile, h = l>>5) holds k = 8h .. 8h+7 (fused_block_early.hip, K16)
                for (int nt = 0; nt < L.cout / 32; ++nt)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int d = 0; d < 4; ++d) {
                            const int nn = nt * 32 + (lane & 31);
                            const size_t at = (size_t)nn * L.cin + 8 * (lane >> 5) + 2 * d;
                            put2(nt, lane, d, w[at] * bn_scale[nn], w[at + 1] * bn_scale[nn]);
                        }
            } else
            for (int nt = 0; nt < ntl; ++nt)
                for (int st = 0; st < kch; ++st)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int d = 0; d < 4; ++d) {
                            float x[2] = {0.f, 0.f};
                            const int nn = nt * 16 + (lane & 15);
                            for (int e = 0; e < 2; ++e) {
                                const int within = (st % spc) * 32 + 8 * (lane >> 4) + 2 * d + e;
                                const int kk = (st / spc) * hc + within;
                                if (nn < L.cout && within < hc) x[e] = w[(size_t)nn * L.cin + kk] * bn_scale[nn];
                            }
                            put2((size_t)nt * kch + st, lane, d, x[0], x[1]);
                        }
            }
        }
        if (L.dst_wrm && L.kind == STEM) {   // row-marching stem (stem_rm.hip): filter / 128 x S as two fp16 pieces in its K-slot order + folded shift + scales
            unsigned *dp = reinterpret_cast<unsigned *>(pk.data() + L.dst_wrm);
            float *fsh = pk.data() + L.dst_wrm + 3 * 2 * 256;
            auto tapw = [&](int co, int ky, int kx, int ci) { return w[co * 27 + ci * 9 + ky * 3 + kx] * bn_scale[co]; };
            float mx = 0.f;
            for (int co = 0; co < 32; ++co)
                for (int t = 0; t < 27; ++t) mx = fmaxf(mx, fabsf(w[co * 27 + t] * bn_scale[co] * (1.0f / 128.0f)));
                        const float S = pow2_scale(mx);
            // K slots of (lane half hh, k16 step st): two pixel quads (R, G, B, -) each -- the LDS ring of stem_rm.hip holds a pixel as four
            // fp16.  (ky, kx) per quad, ky < 0 = zero weights: half 0 kernel row 0 and pixels 0, 1 of row 1; half 1 row 2 and pixel 2 of row 1
            static const int quad_tap[2][3][2][2] = {{{{0, 0}, {0, 1}}, {{0, 2}, {1, 0}}, {{1, 1}, {-1, 0}}},
                                                     {{{2, 0}, {2, 1}}, {{2, 2}, {1, 2}}, {{-1, 0}, {-1, 0}}}};
            for (int st = 0; st < 3; ++st)
                for (int lane = 0; lane < 64; ++lane)
                    for (int d = 0; d < 4; ++d) {
                        float x[2];
                        const int co = lane & 31, hh = lane >> 5;
                        for (int e = 0; e < 2; ++e) {
                            const int slot = 2 * d + e, qd = slot >> 2, ci = slot & 3;
                            const int ky = quad_tap[hh][st][qd][0], kx = quad_tap[hh][st][qd][1];
                            const float v = (ky >= 0 && ci < 3) ? tapw(co, ky, kx, ci) : 0.f;
                            x[e] = v * (1.0f / 128.0f) * S;           // powers of two: exact
                        }
                        const unsigned a0 = f16_rtz(x[0]), a1 = f16_rtz(x[1]);
                        const unsigned b0 = f16_rtz(x[0] - f16_value(a0)), b1 = f16_rtz(x[1] - f16_value(a1));
                        dp[((size_t)(st * 2 + 0) * 64 + lane) * 4 + d] = a0 | (a1 << 16);
                        dp[((size_t)(st * 2 + 1) * 64 + lane) * 4 + d] = b0 | (b1 << 16);
                    }
            for (int co = 0; co < 32; ++co) {
                double sum = 0;
                for (int t = 0; t < 27; ++t) sum += (double)(w[co * 27 + t] * bn_scale[co]);
                fsh[co] = (float)((double)(beta[co] - mean[co] * bn_scale[co]) - 255.0 / 256.0 * sum);
            }
            fsh[32] = S; fsh[33] = 1.0f / S; fsh[34] = 6.0f * S;
            // second set, for normalised fp32 crops (stem_rm.hip F32): the BN-folded filter itself x its own power of two, the plain BN shift
            {
                unsigned *dp2 = dp + syn::rm_stem_set_dwords();
                float *fsh2 = fsh + syn::rm_stem_set_dwords();
                float mx2 = 0.f;
                for (int co = 0; co < 32; ++co)
                    for (int t = 0; t < 27; ++t) mx2 = fmaxf(mx2, fabsf(w[co * 27 + t] * bn_scale[co]));
                const float S2 = pow2_scale(mx2);
                for (int st = 0; st < 3; ++st)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int d = 0; d < 4; ++d) {
                            float x[2];
                            const int co = lane & 31, hh = lane >> 5;
                            for (int e = 0; e < 2; ++e) {
                                const int slot = 2 * d + e, qd = slot >> 2, ci = slot & 3;
                                const int ky = quad_tap[hh][st][qd][0], kx = quad_tap[hh][st][qd][1];
                                x[e] = ((ky >= 0 && ci < 3) ? tapw(co, ky, kx, ci) : 0.f) * S2;
                            }
                            const unsigned a0 = f16_rtz(x[0]), a1 = f16_rtz(x[1]);
                            const unsigned b0 = f16_rtz(x[0] - f16_value(a0)), b1 = f16_rtz(x[1] - f16_value(a1));
                            dp2[((size_t)(st * 2 + 0) * 64 + lane) * 4 + d] = a0 | (a1 << 16);
                            dp2[((size_t)(st * 2 + 1) * 64 + lane) * 4 + d] = b0 | (b1 << 16);
                        }
                for (int co = 0; co < 32; ++co) fsh2[co] = beta[co] - mean[co] * bn_scale[co];
                fsh2[32] = S2; fsh2[33] = 1.0f / S2; fsh2[34] = 6.0f * S2;
            }
        } else if (L.dst_wrm) {          // row-marching early blocks: v_mfma_f32_32x32x16_* fragments (syn_internal.h)
            unsigned *dp = reinterpret_cast<unsigned *>(pk.data() + L.dst_wrm);
            auto split = [](float x, unsigned (&pc)[3]) {
                for (int i = 0; i < 3; ++i) {
                    unsigned u; memcpy(&u, &x, 4); u &= 0xffff0000u;
                    float hf; memcpy(&hf, &u, 4);
                    pc[i] = u >> 16; x -= hf;
                }
            };
            const bool expand = L.relu6 != 0;
            const bool b3 = false;                      // (every row-marching kernel takes two fp16 pieces scaled by S)
            float S = 1.0f;
            if (!b3) {
                float mx = 0.f;
                for (int nn = 0; nn < L.cout; ++nn)
                    for (int k = 0; k < L.cin; ++k) mx = fmaxf(mx, fabsf(w[(size_t)nn * L.cin + k] * bn_scale[nn]));
                                S = pow2_scale(mx);
                pk[L.dst_scl] = S; pk[L.dst_scl + 1] = 1.0f / S; pk[L.dst_scl + 2] = 6.0f * S;
            }
            const int hid = expand ? L.cout : L.cin, ng = (hid + 31) / 32, ks = expand ? (L.cin + 15) / 16 : 2;
            for (int g = 0; g < ng; ++g)
                for (int st = 0; st < ks; ++st)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int d = 0; d < 4; ++d) {
                            unsigned pc[2][3] = {{0, 0, 0}, {0, 0, 0}};
                            float v2[2] = {0.f, 0.f};
                            const int i = lane & 31, hh = lane >> 5;
                            for (int e = 0; e < 2; ++e) {
                                const int sl = 2 * d + e;
                                float v = 0.f;
                                if (expand) {
                                    const int ch = 32 * g + i, k = 16 * st + 8 * hh + sl;
                                    if (ch < L.cout && k < L.cin) v = w[(size_t)ch * L.cin + k] * bn_scale[ch];
                                } else {
                                    const int c = 32 * g + 16 * st + 8 * (sl >> 2) + 4 * hh + (sl & 3);
                                    if (i < L.cout && c < L.cin) v = w[(size_t)i * L.cin + c] * bn_scale[i];
                                }
                                split(v, pc[e]);
                                v2[e] = v * S;
                            }
                            if (b3) {
                                for (int pcs = 0; pcs < 3; ++pcs)
                                    dp[(((size_t)(g * ks + st) * 3 + pcs) * 64 + lane) * 4 + d] = pc[0][pcs] | (pc[1][pcs] << 16);
                            } else {
                                const unsigned a0 = f16_rtz(v2[0]), a1 = f16_rtz(v2[1]);
                                const unsigned b0 = f16_rtz(v2[0] - f16_value(a0)), b1 = f16_rtz(v2[1] - f16_value(a1));
                                dp[(((size_t)(g * ks + st) * 2 + 0) * 64 + lane) * 4 + d] = a0 | (a1 << 16);
                                dp[(((size_t)(g * ks + st) * 2 + 1) * 64 + lane) * 4 + d] = b0 | (b1 << 16);
                            }
                        }
        }
        for (int c = 0; c < L.cout; ++c) {
            pk[L.dst_scale + c] = bn_scale[c];
            pk[L.dst_shift + c] = beta[c] - mean[c] * bn_scale[c];
        }
    }
    for (size_t li = 0; li + 2 < n.layers.size(); ++li) {      // fused_block_lb.hip (features.8-13): fp16 x2 fragments + per-group constants
        const Layer &L = n.layers[li], &D = n.layers[li + 1], &Pj = n.layers[li + 2];
        if (!L.dst_tlb && !L.dst_glb) continue;
        // x = a + b with a = fp16(x) and b = fp16(x - a) (both toward zero) keeps 22 significant bits: fp16 x fp16 products are exact in
        // fp32, a1 a2 + a1 b2 + b1 a2 misses b1 b2 <= 2^-22.  fp16's narrow exponent wants operands near the top of its range, so
        // every GEMM operand is scaled by a power of two (exact), the weights per layer such that max |w| lands in [2^13, 2^14):
        //   X16 = 16 x;  D = 16 Se (We x + shift);  E = med3(D, 0, 96 Se);  O16 = 16 dshift + sum (taps / Se) E;  B = med3(O16, 0, 96)
        //   acc = 16 Sp (Wp o);  y = acc / (16 Sp) + pshift (+ x)
        auto scaled = [&](const Layer &P, std::vector<float> &v) {
            const float *w = flat + P.src_w;
            const float *gamma = w + (size_t)P.cout * P.cin, *var = gamma + 3 * (size_t)P.cout;
            v.resize((size_t)P.cout * P.cin);
            float mx = 0.f;
            for (int nn = 0; nn < P.cout; ++nn) {
                const float sc = gamma[nn] * (1.0f / sqrtf(var[nn] + 1e-5f));
                for (int k = 0; k < P.cin; ++k) { v[(size_t)nn * P.cin + k] = w[(size_t)nn * P.cin + k] * sc; mx = fmaxf(mx, fabsf(v[(size_t)nn * P.cin + k])); }
            }
            const float S = pow2_scale(mx);                                // mx * S in [2^13, 2^14)
            for (float &x : v) x *= S;
            return S;
        };
        auto put = [](unsigned *dp, size_t frag, int lane, int d, float x0, float x1) {      // fragment = [piece 2][lane 64][4 dwords]
            const unsigned a0 = f16_rtz(x0), a1 = f16_rtz(x1);
            const unsigned b0 = f16_rtz(x0 - f16_value(a0)), b1 = f16_rtz(x1 - f16_value(a1));
            dp[((frag * 2 + 0) * 64 + lane) * 4 + d] = a0 | (a1 << 16);
            dp[((frag * 2 + 1) * 64 + lane) * 4 + d] = b0 | (b1 << 16);
        };
        std::vector<float> we, wp;
        const float Se = scaled(L, we), Sp = scaled(Pj, wp);
        const int hid = L.cout, cin = L.cin, cout = Pj.cout, ke = cin / 32, ng = hid / 32, mtn = cout / 16;
        // expand fragment (hidden tile nt, k32 step kc), project fragment (group g, out tile mt), constants of group g
        auto put_e = [&](unsigned *dst, int nt, int kc) {
            for (int lane = 0; lane < 64; ++lane)
                for (int d = 0; d < 4; ++d) {
                    const size_t at = (size_t)(nt * 16 + (lane & 15)) * cin + 32 * kc + 8 * (lane >> 4) + 2 * d;
                    put(dst, 0, lane, d, we[at], we[at + 1]);
                }
        };
        auto put_p = [&](unsigned *dst, int g, int mt) {
            for (int lane = 0; lane < 64; ++lane)
                for (int d = 0; d < 4; ++d) {
                    const int nn = 16 * mt + (lane & 15), kg = lane >> 4;
                    float x[2];
                    for (int e = 0; e < 2; ++e) {
                        const int sl = 2 * d + e;
                        x[e] = wp[(size_t)nn * hid + 32 * g + (sl < 4 ? 4 * kg + sl : 16 + 4 * kg + sl - 4)];
                    }
                    put(dst, 0, lane, d, x[0], x[1]);
                }
        };
        // round 4: ReLU6 through clamp modifiers -- E' = clamp(D / (96 Se)) = relu6 / 6, O' = dshift / 6 + sum taps E' (the PLAIN filter),
        // B' = clamp(O') = relu6 / 6 in [0, 1]; acc = (Sp / 6) (Wp o);  y = acc (6 / Sp) + pshift (+ x)
        auto put_t = [&](float *tb, int g) {
            for (int c = 0; c < 32; ++c) {
                for (int k = 0; k < 9; ++k) tb[k * 32 + c] = pk[D.dst_wpk + (size_t)k * hid + 32 * g + c];
                tb[9 * 32 + c] = pk[D.dst_shift + 32 * g + c] * (1.0f / 6.0f);
                tb[10 * 32 + c] = 16.0f * Se * pk[L.dst_shift + 32 * g + c];
            }
        };
        if (L.dst_glb) {             // fused_block_lb4.hip: per group [We: tile 2][k32][piece] | [Wp: out tile][piece] | 12 x 32 constants (+ pad to 2 KB)
            const size_t grp = syn::lb4_group_dwords(cin, cout);
            for (int g = 0; g < ng; ++g) {
                unsigned *base = reinterpret_cast<unsigned *>(pk.data() + L.dst_glb) + (size_t)g * grp;
                for (int t = 0; t < 2; ++t)
                    for (int kc = 0; kc < ke; ++kc) put_e(base + (size_t)(t * ke + kc) * 512, 2 * g + t, kc);
                unsigned *bp = base + (size_t)2 * ke * 512;
                for (int mt = 0; mt < mtn; ++mt) put_p(bp + (size_t)mt * 512, g, mt);
                float *tb = reinterpret_cast<float *>(bp + (size_t)mtn * 512);
                put_t(tb, g);
                if (g == 0) { tb[11 * 32 + 0] = 1.0f / (96.0f * Se); tb[11 * 32 + 1] = 6.0f / Sp; }
            }
            continue;
        }
        unsigned *de = reinterpret_cast<unsigned *>(pk.data() + L.dst_weh);        // [hidden tile 16][k32 step][piece][lane][4]: lane (m, kg) holds k = 32 kc + 8 kg + e
        for (int nt = 0; nt < hid / 16; ++nt)
            for (int kc = 0; kc < ke; ++kc) put_e(de + (size_t)(nt * ke + kc) * 512, nt, kc);
        unsigned *dq = reinterpret_cast<unsigned *>(pk.data() + Pj.dst_wlb);       // [group][out tile][piece][lane][4], K order of syn_internal.h
        for (int g = 0; g < ng; ++g)
            for (int mt = 0; mt < mtn; ++mt) put_p(dq + (size_t)(g * mtn + mt) * 512, g, mt);
        float *tb = pk.data() + L.dst_tlb;
        for (int g = 0; g < ng; ++g) put_t(tb + (size_t)g * 12 * 32, g);
        tb[11 * 32 + 0] = 1.0f / (96.0f * Se);      // scaled expand output -> relu6 / 6 (with the clamp modifier)
        tb[11 * 32 + 1] = 6.0f / Sp;                // project accumulator (of relu6 / 6 activations) -> output
    }
    {   // features.18 (BN scale folded in), scaled by S = 2^e to max |w| in [2^13, 2^14) and split into two fp16 pieces per weight,
        // lane-ordered for v_mfma_f32_16x16x32_f16: [n_tile 80][k_chunk 10][piece 2][lane 64][4 dwords], lane (r16, g) holds
        // k = 32*kc + 8*g + e, e = 0..7, two fp16 per dword (even e in the low half); then {S, 1/S}
        const Layer &L = n.layers.back();
        const float *w = flat + L.src_w;
        const float *gamma = w + (size_t)L.cout * L.cin, *var = gamma + 3 * (size_t)L.cout;
        unsigned *dp = reinterpret_cast<unsigned *>(pk.data() + n.dst_head_f16);
        std::vector<float> sc(L.cout);
        float mx = 0.f;
        for (int nn = 0; nn < L.cout; ++nn) {
            sc[nn] = gamma[nn] * (1.0f / sqrtf(var[nn] + 1e-5f));
            for (int k = 0; k < L.cin; ++k) mx = fmaxf(mx, fabsf(w[(size_t)nn * L.cin + k] * sc[nn]));
        }
                const float S = pow2_scale(mx);
        pk[n.dst_head_f16 + (size_t)80 * 10 * 2 * 256] = S;
        pk[n.dst_head_f16 + (size_t)80 * 10 * 2 * 256 + 1] = 1.0f / S;
        for (int nt = 0; nt < 80; ++nt)
            for (int kc = 0; kc < 10; ++kc)
                for (int lane = 0; lane < 64; ++lane)
                    for (int d = 0; d < 4; ++d) {
                        const int nn = nt * 16 + (lane & 15), k0 = kc * 32 + 8 * (lane >> 4) + 2 * d;
                        const float x0 = w[(size_t)nn * L.cin + k0] * sc[nn] * S, x1 = w[(size_t)nn * L.cin + k0 + 1] * sc[nn] * S;
                        const unsigned a0 = f16_rtz(x0), a1 = f16_rtz(x1);
                        const unsigned b0 = f16_rtz(x0 - f16_value(a0)), b1 = f16_rtz(x1 - f16_value(a1));
                        dp[(((size_t)(nt * 10 + kc) * 2 + 0) * 64 + lane) * 4 + d] = a0 | (a1 << 16);
                        dp[(((size_t)(nt * 10 + kc) * 2 + 1) * 64 + lane) * 4 + d] = b0 | (b1 << 16);
                    }
    }
    // heads: ori[12] | shape[40] | exp[10] concatenated in that order (mobilenetv2_backbone.py:184-188)
    {
        const float *src = flat + n.src_fc;
        static const int hn[3] = {12, 40, 10};
        int row = 0;
        for (int k = 0; k < 3; ++k) {
            memcpy(pk.data() + n.dst_fc_w + (size_t)row * 1280, src, sizeof(float) * hn[k] * 1280);
            src += (size_t)hn[k] * 1280;
            memcpy(pk.data() + n.dst_fc_b + row, src, sizeof(float) * hn[k]);
            src += hn[k];
            row += hn[k];
        }
    }
}

int syn_load_backbone(syn_handle *h, const float *flat, size_t n_floats) {
    if (!h || !flat) return fail(SYN_ERR_INVALID, "syn_load_backbone: NULL argument");
    const Net &n = net();
    if (n_floats != n.flat_count)
        return fail(SYN_ERR_INVALID, "syn_load_backbone: got %zu floats, the MobileNetV2 backbone has %zu", n_floats, n.flat_count);
    std::vector<float> pk;
    pack_backbone_mbv2(flat, pk);
    DeviceGuard g(h->device);
    if (h->d_backbone && h->arch != 0) { HIP_TRY(hipDeviceSynchronize()); HIP_TRY(hipFree(h->d_backbone)); h->d_backbone = nullptr; }
    if (!h->d_backbone) HIP_TRY(hipMalloc((void **)&h->d_backbone, n.packed_count * sizeof(float)));
    HIP_TRY(hipMemcpy(h->d_backbone, pk.data(), n.packed_count * sizeof(float), hipMemcpyHostToDevice));
    h->arch = 0;
    memcpy(&h->ri, pk.data() + n.dst_range, sizeof h->ri);
    return SYN_OK;
}

// include/synergy_hip.h: switch the handle between the default fp16x2 schedule (2) and the exact fp32-MFMA cross-check schedules (1, 0)
int syn_set_schedule(syn_handle *h, int fusion) {
    if (!h) return fail(SYN_ERR_INVALID, "syn_set_schedule: NULL handle");
    if (fusion < 0 || fusion > 2) return fail(SYN_ERR_INVALID, "syn_set_schedule: schedule %d (0 per-layer fp32, 1 fused fp32-MFMA, 2 fused fp16x2)", fusion);
    const int prev = h->fusion;
    h->fusion = fusion;
    return prev;
}

// Verdict of the load-time range analysis (see analyze_mbv2_ranges) as text + counts; include/synergy_hip.h.
int syn_numerics_report(syn_handle *h, char *buf, size_t n) {
    if (!h) return fail(SYN_ERR_INVALID, "syn_numerics_report: NULL handle");
    std::string out;
    char line[256];
    int n_fallback = 0;
    if (!h->d_backbone) out = "no backbone loaded\n";
    else if (is_mb1(h->arch) || is_gn(h->arch) || is_rs(h->arch) || is_bb(h->arch)) {
        snprintf(line, sizeof line, "%s: every product is exact fp32 (fp32-input MFMA, fp32 depthwise): no fp16 operand, nothing to prove or guard\n", arch_name(h->arch));
        out = line;
    }
    else if (h->arch == 1) {
        for (int i = 0; i < 64; ++i) n_fallback += (h->resnet_w_unsafe[i >> 5] >> (i & 31)) & 1u;
        snprintf(line, sizeof line, "resnet50: %d convolution(s) fail the fp16x2 weight criterion -> fp32-MFMA kernel; activations (ReLU) have no static bound: "
                 "guarded at run time (syn_backbone_range_status)%s\n", n_fallback, h->resnet_fp32 ? "; the guard has switched this handle to fp32-MFMA convolutions" : "");
        out = line;
        if (h->resnet_fp32) n_fallback = 53;
    }
    else {
        const RangeInfo &r = h->ri;
        for (int f = 0; f <= 18; ++f) {
            if (f == 1) continue;
            const bool b1 = (r.unsafe1 >> f) & 1u, b16 = ((r.unsafe16 | r.unsafe1) >> f) & 1u, uses16 = f >= 7 && f <= 17;
            const char *sched = b1 ? "fp32-MFMA (exact) kernel" : (uses16 && b16) ? "fp16x2 tiled kernel, input scale 1" : "fp16x2";
            if (b1 || (uses16 && b16)) ++n_fallback;
            snprintf(line, sizeof line, "features.%s%d: input bound %.4g, min weighted-mean bound %.4g, weight criterion %.3g x threshold -> %s\n",
                     f == 0 ? "0-" : "", f == 0 ? 1 : f, (double)r.in_bound[f], (double)r.min_wmean[f], (double)r.w_relerr[f], sched);
            out += line;
        }
        if (!h->range_guard) out += "SYNERGY_HIP_RANGE_GUARD=0: the verdict is NOT applied\n";
    }
    if (buf && n) { snprintf(buf, n, "%s", out.c_str()); }
    return n_fallback;
}

// resnet50 run-time range guard (see run_resnet50): synchronises the device, copies max |x| of every guarded tensor of the LAST
// forward into layer_max[0 .. max_layers) (slot 0 = max-pool output, 1 + i = conv i in state_dict order; unguarded slots read 1)
// and returns how many left the fp16 window.  fallback != 0 and a violation: the handle runs the exact fp32-MFMA convolutions
// from now on (sticky until the next syn_load_backbone_resnet50 / syn_import_constants).  mobilenet_v2 handles return 0.
int syn_backbone_range_status(syn_handle *h, float *layer_max, int max_layers, int fallback) {
    if (!h) return fail(SYN_ERR_INVALID, "syn_backbone_range_status: NULL handle");
    if (h->arch != 1 || !h->d_range) return 0;
    DeviceGuard g(h->device);
    float st[64];
    HIP_TRY(hipDeviceSynchronize());
    if (!h->guard_armed) {          // the last forward ran the exact convolutions (or unguarded): the array still holds an EARLIER forward's maxima
        for (int i = 0; layer_max && i < max_layers && i < 64; ++i) layer_max[i] = 1.0f;
        return 0;
    }
    {
        std::vector<float> raw(kRangeFloats);
        HIP_TRY(hipMemcpy(raw.data(), h->d_range, kRangeFloats * sizeof(float), hipMemcpyDeviceToHost));
        for (int t = 0; t < 64; ++t) {
            st[t] = 0.f;
            for (int i = 0; i < syn::kRangeSub; ++i) st[t] = fmaxf(st[t], raw[((size_t)t * syn::kRangeSub + i) * syn::kRangeStride]);
        }
    }
    int bad = 0;
    for (int i = 0; i < kResnetStat; ++i) bad += !(st[i] <= syn::kRangeHi) || !(st[i] >= syn::kRangeLo);
    for (int i = 0; layer_max && i < max_layers && i < 64; ++i) layer_max[i] = st[i];
    if (bad && fallback) {
        if (!h->resnet_fp32) h->range_events += 1;
        h->resnet_fp32 = 1;
        if (h->guard_word) *(volatile unsigned *)h->guard_word = 0;      // (the device is idle: the word of this forward has landed)
    }
    return bad;
}

int syn_backbone_range_events(syn_handle *h) {
    if (!h) return fail(SYN_ERR_INVALID, "syn_backbone_range_events: NULL handle");
    return h->range_events;
}

size_t syn_resnet50_flat_count(void) { return resnet50().flat_count; }
double syn_resnet50_flops_per_face(void) { return resnet50().flops; }

static void pack_backbone_resnet50(const float *flat, std::vector<float> &pk) {
    const ResNet50 &n = resnet50();
    pk.assign(n.packed_count, 0.f);
    for (const RConv &c : n.convs) {
        const float *w = flat + c.src_w;
        const size_t wn = (size_t)c.cout * c.cin * c.k * c.k;
        const float *gamma = w + wn, *beta = gamma + c.cout, *mean = beta + c.cout, *var = mean + c.cout;
        float *dw = pk.data() + c.dst_w;
        const int taps = c.k * c.k;
        if (c.cin == 3) {                 // stem: [64][3][7][7] -> [ci*49 + ky*7 + kx][64]
            for (int co = 0; co < c.cout; ++co)
                for (int t = 0; t < 3 * taps; ++t) dw[(size_t)t * c.cout + co] = w[(size_t)co * 3 * taps + t];
        } else {                          // [N][C][ky][kx] -> [N][(ky*KW + kx)*C + c]
            for (int nn = 0; nn < c.cout; ++nn)
                for (int ci = 0; ci < c.cin; ++ci)
                    for (int t = 0; t < taps; ++t)
                        dw[(size_t)nn * taps * c.cin + (size_t)t * c.cin + ci] = w[((size_t)nn * c.cin + ci) * taps + t];
        }
        if (c.dst_wrm) {   // 7x7 stem on the fp16 matrix instructions: K order / folding documented in syn_internal.h
            unsigned *dp = reinterpret_cast<unsigned *>(pk.data() + c.dst_wrm);
            float *fsh = pk.data() + c.dst_wrm + 2 * 10 * 2 * 256;
            float mx = 0.f;
            for (int co = 0; co < 64; ++co) {
                const float a = gamma[co] * (1.0f / sqrtf(var[co] + 1e-5f));
                for (int t = 0; t < 147; ++t) mx = fmaxf(mx, fabsf(w[(size_t)co * 147 + t] * a * (1.0f / 128.0f)));
            }
                        const float S = pow2_scale(mx);
            for (int G = 0; G < 2; ++G)
                for (int st = 0; st < 10; ++st)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int d = 0; d < 4; ++d) {
                            float x[2] = {0.f, 0.f};
                            const int co = 32 * G + (lane & 31), hh = lane >> 5;
                            for (int e = 0; e < 2; ++e) {
                                const int kk = 16 * st + 8 * hh + 2 * d + e, ky = kk / 22, m = kk % 22;
                                if (kk < 154 && m >= 1) {
                                    const int kx = (m - 1) / 3, ci = (m - 1) % 3;
                                    const float a = gamma[co] * (1.0f / sqrtf(var[co] + 1e-5f));
                                    x[e] = w[(size_t)co * 147 + ci * 49 + ky * 7 + kx] * a * (1.0f / 128.0f) * S;
                                }
                            }
                            const unsigned a0 = f16_rtz(x[0]), a1 = f16_rtz(x[1]);
                            const unsigned b0 = f16_rtz(x[0] - f16_value(a0)), b1 = f16_rtz(x[1] - f16_value(a1));
                            dp[((size_t)((G * 10 + st) * 2 + 0) * 64 + lane) * 4 + d] = a0 | (a1 << 16);
                            dp[((size_t)((G * 10 + st) * 2 + 1) * 64 + lane) * 4 + d] = b0 | (b1 << 16);
                        }
            for (int co = 0; co < 64; ++co) {
                const float a = gamma[co] * (1.0f / sqrtf(var[co] + 1e-5f));
                double sum = 0;
                for (int t = 0; t < 147; ++t) sum += (double)(w[(size_t)co * 147 + t] * a);
                fsh[co] = (float)((double)(beta[co] - mean[co] * a) - 255.0 / 256.0 * sum);
            }
            fsh[64] = S; fsh[65] = 1.0f / S;
        }
        if (c.dst_w3) {   // [N][tap*Cin + ci] x S -> [n_tile][tap*Cin/32 + kc][piece 2][lane][4 dwords], {S, 1/S}: S = 2^e, max |w| S in [2^13, 2^14)
            unsigned *dp = reinterpret_cast<unsigned *>(pk.data() + c.dst_w3);
            const int kch = c.cin / 32, steps = taps * kch, K = taps * c.cin;
            float mx = 0.f;
            for (size_t i = 0; i < (size_t)c.cout * K; ++i) mx = fmaxf(mx, fabsf(dw[i]));
                        const float S = pow2_scale(mx);
            float *tail = pk.data() + c.dst_w3 + (size_t)(c.cout / 16) * steps * 512;
            tail[0] = S; tail[1] = 1.0f / S;
            {   // weight criterion of analyze_mbv2_ranges on the BN-less weights (the BN scale is applied in fp32 by the epilogue):
                // a row whose pieces err by more than 2^-17 of its L1 norm sends the whole convolution to the fp32-MFMA kernel
                bool bad = !std::isfinite(mx);
                for (int nn = 0; nn < c.cout && !bad; ++nn) {
                    double err = 0, mag = 0;
                    for (int k = 0; k < K; ++k) {
                        const float x = dw[(size_t)nn * K + k] * S;
                        const unsigned a = f16_rtz(x), b = f16_rtz(x - f16_value(a));
                        err += fabs((double)x - (double)f16_value(a) - (double)f16_value(b));
                        mag += fabs((double)x);
                    }
                    bad = err > mag * 7.62939453125e-6;
                }
                if (bad) {
                    const int ci = (int)(&c - n.convs.data());
                    uint32_t *m = reinterpret_cast<uint32_t *>(pk.data() + n.dst_range);
                    m[ci >> 5] |= 1u << (ci & 31);
                }
            }
            for (int nt = 0; nt < c.cout / 16; ++nt)
                for (int st = 0; st < steps; ++st)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int d = 0; d < 4; ++d) {
                            // MFMA row rho = lane & 15 of tile nt: the output channel in PAIR ORDER (resnet_kernels.hip: a lane's accumulators of tiles
                            // 2 b, 2 b + 1 are eight consecutive channels = one 16-byte piece of the pair format)
                            const int rho = lane & 15;
                            const int nn = 32 * (nt >> 1) + 8 * (rho >> 2) + 4 * (nt & 1) + (rho & 3);
                            const int k0 = (st / kch) * c.cin + (st % kch) * 32 + 8 * (lane >> 4) + 2 * d;
                            const float x0 = dw[(size_t)nn * K + k0] * S, x1 = dw[(size_t)nn * K + k0 + 1] * S;
                            const unsigned a0 = f16_rtz(x0), a1 = f16_rtz(x1);
                            const unsigned b0 = f16_rtz(x0 - f16_value(a0)), b1 = f16_rtz(x1 - f16_value(a1));
                            dp[((((size_t)nt * steps + st) * 2 + 0) * 64 + lane) * 4 + d] = a0 | (a1 << 16);
                            dp[((((size_t)nt * steps + st) * 2 + 1) * 64 + lane) * 4 + d] = b0 | (b1 << 16);
                        }
        }
        if (c.dst_w1f) {   // the same fragments for conv_c3f_kernel, step-major: [k32 step][tile][piece 2][lane][4] (a copy of dst_w3's [tile][step][...])
            unsigned *dp = reinterpret_cast<unsigned *>(pk.data() + c.dst_w1f);
            const unsigned *sp = reinterpret_cast<const unsigned *>(pk.data() + c.dst_w3);
            const int nt1 = c.cout / 16, kch1 = c.cin / 32;
            for (int kc = 0; kc < kch1; ++kc)
                for (int i1 = 0; i1 < nt1; ++i1)
                    memcpy(dp + ((size_t)kc * nt1 + i1) * 512, sp + ((size_t)i1 * kch1 + kc) * 512, 512 * sizeof(unsigned));
        }
        for (int ch = 0; ch < c.cout; ++ch) {
            const float a = gamma[ch] * (1.0f / sqrtf(var[ch] + 1e-5f));
            pk[c.dst_scale + ch] = a;
            pk[c.dst_shift + ch] = beta[ch] - mean[ch] * a;
        }
    }
    // conv3 + stride-2 downsample branch as ONE GEMM (resnet_kernels.hip DUAL): out = relu(a3 (W3 t) + sh3 + ad (Wd x) + shd) = relu([a3 W3 | ad Wd] [t ; x] + (sh3 + shd)):
    // the BatchNorm scales folded into the rows, one power of two S for the combined matrix, rows in pair order, K = conv3's channels then the branch's
    for (const RBlock &b : n.blocks) {
        if (!b.dst_w3d) continue;
        const RConv &c3 = n.convs[b.c3], &cd = n.convs[b.ds];
        const int N = c3.cout, K1 = c3.cin, K2 = cd.cin, K = K1 + K2, steps = K / 32;
        std::vector<float> wf((size_t)N * K);
        float mx = 0.f;
        for (int nn = 0; nn < N; ++nn) {
            const float a3 = pk[c3.dst_scale + nn], ad = pk[cd.dst_scale + nn];
            for (int k = 0; k < K1; ++k) wf[(size_t)nn * K + k] = pk[c3.dst_w + (size_t)nn * K1 + k] * a3;
            for (int k = 0; k < K2; ++k) wf[(size_t)nn * K + K1 + k] = pk[cd.dst_w + (size_t)nn * K2 + k] * ad;
            pk[b.dst_ones + nn] = 1.0f;
            pk[b.dst_shiftd + nn] = pk[c3.dst_shift + nn] + pk[cd.dst_shift + nn];
        }
        for (float v : wf) mx = fmaxf(mx, fabsf(v));
        const float S = pow2_scale(mx);
        unsigned *dp = reinterpret_cast<unsigned *>(pk.data() + b.dst_w3d);
        float *tail = pk.data() + b.dst_w3d + (size_t)(N / 16) * steps * 512;
        tail[0] = S; tail[1] = 1.0f / S;
        bool bad = !std::isfinite(mx);
        for (int nn = 0; nn < N && !bad; ++nn) {
            double err = 0, mag = 0;
            for (int k = 0; k < K; ++k) {
                const float x = wf[(size_t)nn * K + k] * S;
                const unsigned a = f16_rtz(x), bb = f16_rtz(x - f16_value(a));
                err += fabs((double)x - (double)f16_value(a) - (double)f16_value(bb));
                mag += fabs((double)x);
            }
            bad = err > mag * 7.62939453125e-6;
        }
        if (bad) reinterpret_cast<uint32_t *>(pk.data() + n.dst_range)[2] |= 1u << b.dual_idx;
        for (int nt = 0; nt < N / 16; ++nt)
            for (int st = 0; st < steps; ++st)
                for (int lane = 0; lane < 64; ++lane)
                    for (int d = 0; d < 4; ++d) {
                        const int rho = lane & 15, nn = 32 * (nt >> 1) + 8 * (rho >> 2) + 4 * (nt & 1) + (rho & 3);
                        const int k0 = st * 32 + 8 * (lane >> 4) + 2 * d;
                        const float x0 = wf[(size_t)nn * K + k0] * S, x1 = wf[(size_t)nn * K + k0 + 1] * S;
                        const unsigned a0 = f16_rtz(x0), a1 = f16_rtz(x1);
                        const unsigned b0 = f16_rtz(x0 - f16_value(a0)), b1 = f16_rtz(x1 - f16_value(a1));
                        dp[((((size_t)nt * steps + st) * 2 + 0) * 64 + lane) * 4 + d] = a0 | (a1 << 16);
                        dp[((((size_t)nt * steps + st) * 2 + 1) * 64 + lane) * 4 + d] = b0 | (b1 << 16);
                    }
    }
    {   // heads: flat order fc_tex, fc_ori, fc_shape, fc_exp (module order, resnet_backbone.py:185-188);
        // packed rows in the cat order ori | shape | exp | tex (:246)
        const float *src = flat + n.src_fc;
        static const int hn[4] = {40, 12, 40, 10};        // tex, ori, shape, exp
        static const int row0[4] = {62, 0, 12, 52};
        for (int k = 0; k < 4; ++k) {
            memcpy(pk.data() + n.dst_fc_w + (size_t)row0[k] * 2048, src, sizeof(float) * hn[k] * 2048);
            src += (size_t)hn[k] * 2048;
            memcpy(pk.data() + n.dst_fc_b + row0[k], src, sizeof(float) * hn[k]);
            src += hn[k];
        }
    }
}

int syn_load_backbone_resnet50(syn_handle *h, const float *flat, size_t n_floats) {
    if (!h || !flat) return fail(SYN_ERR_INVALID, "syn_load_backbone_resnet50: NULL argument");
    const ResNet50 &n = resnet50();
    if (n_floats != n.flat_count)
        return fail(SYN_ERR_INVALID, "syn_load_backbone_resnet50: got %zu floats, ResNet-50 has %zu", n_floats, n.flat_count);
    std::vector<float> pk;
    pack_backbone_resnet50(flat, pk);
    if (int rc = install_backbone(h, 1, pk.data(), n.packed_count)) return rc;
    memcpy(h->resnet_w_unsafe, pk.data() + n.dst_range, sizeof h->resnet_w_unsafe);
    return SYN_OK;
}

// ---- MobileNetV1: flat = the module's state_dict order without num_batches_tracked (synergynet_amd.synergy3DMM.mobilenet1_keys) ----
size_t syn_mobilenet1_flat_count(int arch) { return is_mb1(arch) ? mb1net(arch).flat_count : 0; }
double syn_mobilenet1_flops_per_face(int arch) { return is_mb1(arch) ? mb1net(arch).flops : 0.0; }

static void pack_backbone_mobilenet1(int arch, const float *flat, std::vector<float> &pk) {
    const Mb1Net &n = mb1net(arch);
    pk.assign(n.packed_count, 0.f);
    pack_conv_t(flat, n.stem, pk);                            // conv1.weight [c0][3][3][3] -> [ci*9 + ky*3 + kx][c0]
    for (const Mb1Block &b : n.blocks) {
        pack_conv_t(flat, b.dw, pk);                          // conv_dw.weight [cin][1][3][3] -> tap-major [9][cin]
        pack_conv(flat, b.pw, pk);                            // conv_sep.weight [cout][cin]: as the kernels read it
    }
    pack_heads(flat, n.fc, pk);      // flat order fc_ori, fc_shape, fc_exp, fc_tex = the cat order (:132-138): rows 0..61 as they come
}

int syn_load_backbone_mobilenet1(syn_handle *h, int arch, const float *flat, size_t n_floats) {
    if (!h || !flat) return fail(SYN_ERR_INVALID, "syn_load_backbone_mobilenet1: NULL argument");
    if (!is_mb1(arch)) return fail(SYN_ERR_INVALID, "syn_load_backbone_mobilenet1: arch=%d (2 mobilenet_1, 3 mobilenet_05, 4 mobilenet_2)", arch);
    const Mb1Net &n = mb1net(arch);
    if (n_floats != n.flat_count)
        return fail(SYN_ERR_INVALID, "syn_load_backbone_mobilenet1: got %zu floats, %s has %zu", n_floats, arch_name(arch), n.flat_count);
    std::vector<float> pk;
    pack_backbone_mobilenet1(arch, flat, pk);
    return install_backbone(h, arch, pk.data(), pk.size());
}

// ---- GhostNet: flat = the module's state_dict order without num_batches_tracked (synergynet_amd.synergy3DMM.ghostnet_keys) ----
size_t syn_ghostnet_flat_count(void) { return gnnet().flat_count; }
double syn_ghostnet_flops_per_face(void) { return gnnet().flops; }

static void pack_backbone_ghostnet(int, const float *flat, std::vector<float> &pk) {
    const GnNet &n = gnnet();
    pk.assign(n.packed_count, 0.f);
    auto conv = [&](const ConvBn &c) { pack_conv(flat, c, pk); };        // [cout][cin]: as the kernels read it
    auto dwc = [&](const ConvBn &d) { pack_conv_t(flat, d, pk); };       // [c][1][k][k] -> tap-major [k*k][c]
    pack_conv_t(flat, n.stem, pk);      // conv_stem.weight [16][3][3][3] -> [ci*9 + ky*3 + kx][16] (launch_mb1_stem's layout)
    for (const GnBlock &b : n.blocks) {
        conv(b.g1p); dwc(b.g1d);
        if (b.stride == 2) dwc(b.dw);
        if (b.se) {
            const float *src = flat + b.src_se;
            const size_t wn = (size_t)b.se * b.mid;
            memcpy(pk.data() + b.dst_rw, src, sizeof(float) * wn);
            memcpy(pk.data() + b.dst_rb, src + wn, sizeof(float) * b.se);
            memcpy(pk.data() + b.dst_ew, src + wn + b.se, sizeof(float) * wn);
            memcpy(pk.data() + b.dst_eb, src + 2 * wn + b.se, sizeof(float) * b.mid);
        }
        conv(b.g2p); dwc(b.g2d);
        if (b.conv_sc) { dwc(b.scd); conv(b.scp); }
    }
    conv(n.last);
    memcpy(pk.data() + n.dst_head_w, flat + n.src_head, sizeof(float) * (size_t)GnNet::kPool * GnNet::kLast);
    memcpy(pk.data() + n.dst_head_b, flat + n.src_head + (size_t)GnNet::kPool * GnNet::kLast, sizeof(float) * GnNet::kPool);
    pack_heads(flat, n.fc, pk);      // flat order classifier_ori, _shape, _exp, _texture = the cat order (:227-231): rows 0..61 as they come
}

int syn_load_backbone_ghostnet(syn_handle *h, const float *flat, size_t n_floats) {
    if (!h || !flat) return fail(SYN_ERR_INVALID, "syn_load_backbone_ghostnet: NULL argument");
    const GnNet &n = gnnet();
    if (n_floats != n.flat_count) return fail(SYN_ERR_INVALID, "syn_load_backbone_ghostnet: got %zu floats, ghostnet has %zu", n_floats, n.flat_count);
    std::vector<float> pk;
    pack_backbone_ghostnet(kArchGhost, flat, pk);
    return install_backbone(h, kArchGhost, pk.data(), pk.size());
}

// ---- ResNeSt-50: flat = the module's state_dict order without num_batches_tracked (synergynet_amd.synergy3DMM.resnest50_keys) ----
size_t syn_resnest50_flat_count(void) { return rsnet().flat_count; }
double syn_resnest50_flops_per_face(void) { return rsnet().flops; }

static void pack_backbone_resnest50(int, const float *flat, std::vector<float> &pk) {
    const RsNet &n = rsnet();
    pk.assign(n.packed_count, 0.f);
    auto conv = [&](const ConvBn &c) { pack_conv(flat, c, pk); };      // 1x1 [cout][cin]: as the kernels read it; 3x3 [n][cg][3][3] -> [n][tap][cg]
    pack_conv_t(flat, n.stem, pk);                            // conv1.0.weight [32][3][3][3] -> [ci*9 + ky*3 + kx][32]
    conv(n.stem2);
    conv(n.stem3);
    for (const RsBlock &b : n.blocks) {
        conv(b.c1);
        conv(b.c2);
        const int C = b.C, I = b.inter;
        const float *w1 = flat + b.src_fc, *b1 = w1 + (size_t)I * C, *bn = b1 + I, *w2 = bn + 4 * (size_t)I, *b2 = w2 + 2 * (size_t)C * I;
        for (int j = 0; j < I; ++j) {
            for (int k = 0; k < C; ++k) pk[b.dst_w1t + (size_t)k * I + j] = w1[(size_t)j * C + k];
            const float sc = bn[j] / sqrtf(bn[3 * I + j] + 1e-5f);
            pk[b.dst_s1 + j] = sc;
            pk[b.dst_h1 + j] = (b1[j] - bn[2 * I + j]) * sc + bn[I + j];      // BN(dot + bias)
        }
        for (int o = 0; o < 2 * C; ++o) {
            for (int k = 0; k < I; ++k) pk[b.dst_w2t + (size_t)k * 2 * C + o] = w2[(size_t)o * I + k];
            pk[b.dst_b2 + o] = b2[o];
        }
        conv(b.c3);
        if (b.down) conv(b.ds);
    }
    pack_heads(flat, n.fc, pk);      // flat order fc_ori, fc_shape, fc_exp, fc_tex; the cat (:320) is ori | shape | exp: rows 0..61 as they come
}

int syn_load_backbone_resnest50(syn_handle *h, const float *flat, size_t n_floats) {
    if (!h || !flat) return fail(SYN_ERR_INVALID, "syn_load_backbone_resnest50: NULL argument");
    const RsNet &n = rsnet();
    if (n_floats != n.flat_count) return fail(SYN_ERR_INVALID, "syn_load_backbone_resnest50: got %zu floats, resnest50 has %zu", n_floats, n.flat_count);
    std::vector<float> pk;
    pack_backbone_resnest50(kArchResnest, flat, pk);
    return install_backbone(h, kArchResnest, pk.data(), pk.size());
}

// ---- resnet18 / resnet34: flat = the module's state_dict order without num_batches_tracked (synergynet_amd.synergy3DMM.resnet_basic_keys) ----
size_t syn_resnet_basic_flat_count(int arch) { return is_bb(arch) ? bbnet(arch).flat_count : 0; }
double syn_resnet_basic_flops_per_face(int arch) { return is_bb(arch) ? bbnet(arch).flops : 0.0; }

static void pack_backbone_resnet_basic(int arch, const float *flat, std::vector<float> &pk) {
    const BbNet &n = bbnet(arch);
    pk.assign(n.packed_count, 0.f);
    pack_conv_t(flat, n.stem, pk);                            // [64][3][7][7] -> [ci*49 + ky*7 + kx][64]
    for (const BbBlock &b : n.blocks) {
        pack_conv(flat, b.c1, pk);                            // [n][cin][3][3] -> [n][tap][cin]
        pack_conv(flat, b.c2, pk);
        if (b.down) pack_conv(flat, b.ds, pk);
    }
    // flat order fc_tex, fc_ori, fc_shape, fc_exp; the forward's cat (:246) is ori | shape | exp | tex and the adapter takes the first 62:
    // rows 0..61 = ori | shape | exp, which n.fc.src points at; fc_tex is not packed
    pack_heads(flat, n.fc, pk);
}

int syn_load_backbone_resnet_basic(syn_handle *h, int arch, const float *flat, size_t n_floats) {
    if (!h || !flat) return fail(SYN_ERR_INVALID, "syn_load_backbone_resnet_basic: NULL argument");
    if (!is_bb(arch)) return fail(SYN_ERR_INVALID, "syn_load_backbone_resnet_basic: arch=%d, expected 10 (resnet18) or 11 (resnet34)", arch);
    const BbNet &n = bbnet(arch);
    if (n_floats != n.flat_count) return fail(SYN_ERR_INVALID, "syn_load_backbone_resnet_basic: got %zu floats, %s has %zu", n_floats, arch_name(arch), n.flat_count);
    std::vector<float> pk;
    pack_backbone_resnet_basic(arch, flat, pk);
    return install_backbone(h, arch, pk.data(), pk.size());
}

static void pack_basis(const float *w_shp, const float *w_exp, const float *u, const float *param_mean, const float *param_std,
                       const int64_t *keypoints, int n_lmk, int n_vert, std::vector<float> &pk) {
    const int nvp = round_up(n_vert, 32), nlp = round_up(n_lmk, 32);
    const size_t total = basis_float_count(nvp, nlp);
    pk.assign(total, 0.f);
    pack_basis_tiles(pk.data(), n_vert, nvp / 32, w_shp, w_exp, u, nullptr);
    // landmark sub-basis: w_*_base = w_*[keypoints], u_base = u[keypoints] (utils/params.py:31-33)
    pack_basis_tiles(pk.data() + (size_t)nvp * 3 * syn::kBasisK, n_lmk, nlp / 32, w_shp, w_exp, u, keypoints);
    float *ms = pk.data() + (size_t)(nvp + nlp) * 3 * syn::kBasisK;
    memcpy(ms, param_mean, sizeof(float) * 62);
    memcpy(ms + 64, param_std, sizeof(float) * 62);
    // fp16 x2 path: EVERY basis column k (and the mean shape u, k = 50) gets its own power of two 2^e_k with max_rows |column| 2^e_k in
    // [2^13, 2^14), so that its entries sit at the top of fp16's exponent range whatever the column's magnitude (BFM-like packs: u ~ 1e5
    // next to PCA directions ~ 1e-3: under ONE common scale the latter fell into fp16 subnormals and kept ~13 bits).  The inverse
    // 2^-e_k is folded into the de-whitening constants of coefficient k (alpha_k 2^-e_k = p (std_k 2^-e_k) + mean_k 2^-e_k: exact, a
    // power of two commutes with the fp32 rounding), the mean shape's coefficient becomes 2^-e_u; the products are unchanged.
    float colscale[51], colinv[51];
    for (int k = 0; k < 51; ++k) {
        float mx = 0.f;
        if (k < 40) { for (size_t r = 0; r < (size_t)3 * n_vert; ++r) mx = fmaxf(mx, fabsf(w_shp[r * 40 + k])); }
        else if (k < 50) { for (size_t r = 0; r < (size_t)3 * n_vert; ++r) mx = fmaxf(mx, fabsf(w_exp[r * 10 + (k - 40)])); }
        else { for (size_t r = 0; r < (size_t)3 * n_vert; ++r) mx = fmaxf(mx, fabsf(u[r])); }
        int ex = 0;
        if (mx > 0.f && std::isfinite(mx)) { (void)frexpf(mx, &ex); ex = 14 - ex; }
        ex = ex < -60 ? -60 : (ex > 60 ? 60 : ex);          // (keeps alpha 2^-e and 2^-e_u comfortably inside fp32)
        colscale[k] = ldexpf(1.0f, ex); colinv[k] = ldexpf(1.0f, -ex);
    }
    float *mcs = ms + 128, *scs = ms + 192;
    memcpy(mcs, param_mean, sizeof(float) * 62);
    memcpy(scs, param_std, sizeof(float) * 62);
    for (int k = 0; k < 50; ++k) { mcs[12 + k] *= colinv[k]; scs[12 + k] *= colinv[k]; }
    mcs[62] = colinv[50];                                   // coefficient of the (scaled) mean shape
    unsigned *b3 = reinterpret_cast<unsigned *>(ms + 256);
    pack_basis_tiles_f16(b3, n_vert, nvp / 32, w_shp, w_exp, u, nullptr, colscale);
    pack_basis_tiles_f16(b3 + (size_t)(nvp / 32) * 3 * syn::kBasisF16, n_lmk, nlp / 32, w_shp, w_exp, u, keypoints, colscale);
}

int syn_load_basis(syn_handle *h, const float *w_shp, const float *w_exp, const float *u, const float *param_mean,
                   const float *param_std, const int64_t *keypoints, int n_lmk, int n_vert) {
    if (!h || !w_shp || !w_exp || !u || !param_mean || !param_std || !keypoints)
        return fail(SYN_ERR_INVALID, "syn_load_basis: NULL argument");
    if (n_vert <= 0 || n_lmk <= 0) return fail(SYN_ERR_INVALID, "syn_load_basis: n_vert=%d n_lmk=%d", n_vert, n_lmk);
    for (int i = 0; i < 3 * n_lmk; ++i)
        if (keypoints[i] < 0 || keypoints[i] >= (int64_t)3 * n_vert)
            return fail(SYN_ERR_INVALID, "syn_load_basis: keypoints[%d]=%lld out of range", i, (long long)keypoints[i]);
    const int nvp = round_up(n_vert, 32), nlp = round_up(n_lmk, 32);
    const size_t total = basis_float_count(nvp, nlp);
    std::vector<float> pk;
    pack_basis(w_shp, w_exp, u, param_mean, param_std, keypoints, n_lmk, n_vert, pk);
    DeviceGuard g(h->device);
    if (h->d_basis && h->basis_floats != total) { HIP_TRY(hipFree(h->d_basis)); h->d_basis = nullptr; }
    if (!h->d_basis) HIP_TRY(hipMalloc((void **)&h->d_basis, total * sizeof(float)));
    HIP_TRY(hipMemcpy(h->d_basis, pk.data(), total * sizeof(float), hipMemcpyHostToDevice));
    h->basis_floats = total; h->n_vert = n_vert; h->n_lmk = n_lmk; h->nvp = nvp; h->nlp = nlp;
    return SYN_OK;
}

namespace {
const std::vector<ArchInfo> &arch_table() {
    static const std::vector<ArchInfo> table = [] {
        std::vector<ArchInfo> t;
        const Net &m = net();
        t.push_back({0, "mobilenet_v2", m.flat_count, m.packed_count, 2 * m.max_io + 2 * m.max_hidden, 1280,
                     [](int, const float *flat, std::vector<float> &pk) { pack_backbone_mbv2(flat, pk); }});
        const ResNet50 &r = resnet50();
        t.push_back({1, "resnet50", r.flat_count, r.packed_count, 4 * r.buf_big + 2 * r.buf_mid, 2048,
                     [](int, const float *flat, std::vector<float> &pk) { pack_backbone_resnet50(flat, pk); }});
        static const char *const mb1_names[3] = {"mobilenet_1", "mobilenet_05", "mobilenet_2"};
        for (int a = kArchMb1First; a <= kArchLast; ++a) {
            const Mb1Net &n = mb1net(a);
            t.push_back({a, mb1_names[a - kArchMb1First], n.flat_count, n.packed_count, n.ws_per_face(), n.pool, pack_backbone_mobilenet1});
        }
        const GnNet &g = gnnet();
        t.push_back({kArchGhost, "ghostnet", g.flat_count, g.packed_count, g.ws_per_face(), GnNet::kPool, pack_backbone_ghostnet});
        const RsNet &s = rsnet();
        t.push_back({kArchResnest, "resnest50", s.flat_count, s.packed_count, s.ws_per_face(), RsNet::kPool, pack_backbone_resnest50});
        for (int a : {kArchRes18, kArchRes34}) {
            const BbNet &n = bbnet(a);
            t.push_back({a, a == kArchRes18 ? "resnet18" : "resnet34", n.flat_count, n.packed_count, n.ws_per_face(), BbNet::kPool,
                         pack_backbone_resnet_basic});
        }
        return t;
    }();
    return table;
}
}  // namespace

// Device-free twins of the constant hand-off: pack the blob syn_export_constants would produce straight from host
// arrays, and run the checks syn_import_constants makes on a host copy of a blob.  No HIP call is made: usable on a machine
// without a GPU (a loader process, or tests/test_dist_cpu.py's gloo ranks).
size_t syn_pack_constants_host_bytes(int arch, int have_backbone, int n_vert, int n_lmk) {
    if (!arch_known(arch)) return 0;
    size_t fl = have_backbone ? backbone_floats(arch) : 0;
    if (n_vert > 0 && n_lmk > 0) fl += basis_float_count(round_up(n_vert, 32), round_up(n_lmk, 32));
    return sizeof(ConstHeader) + fl * sizeof(float);
}

int syn_pack_constants_host(int arch, const float *backbone_flat, size_t n_floats, const float *w_shp, const float *w_exp, const float *u,
                            const float *param_mean, const float *param_std, const int64_t *keypoints, int n_lmk, int n_vert,
                            void *host_dst, size_t bytes) {
    if (!host_dst) return fail(SYN_ERR_INVALID, "syn_pack_constants_host: NULL destination");
    if (!arch_known(arch)) return fail(SYN_ERR_INVALID, "syn_pack_constants_host: arch=%d", arch);
    const bool has_bb = backbone_flat != nullptr, has_basis = w_shp != nullptr;
    if (has_bb && n_floats != backbone_flat_floats(arch))
        return fail(SYN_ERR_INVALID, "syn_pack_constants_host: got %zu backbone floats", n_floats);
    if (has_basis) {
        if (!w_exp || !u || !param_mean || !param_std || !keypoints || n_vert <= 0 || n_lmk <= 0)
            return fail(SYN_ERR_INVALID, "syn_pack_constants_host: incomplete basis arguments");
        for (int i = 0; i < 3 * n_lmk; ++i)
            if (keypoints[i] < 0 || keypoints[i] >= (int64_t)3 * n_vert)
                return fail(SYN_ERR_INVALID, "syn_pack_constants_host: keypoints[%d]=%lld out of range", i, (long long)keypoints[i]);
    }
    const size_t need = syn_pack_constants_host_bytes(arch, has_bb, has_basis ? n_vert : 0, has_basis ? n_lmk : 0);
    if (bytes < need) return fail(SYN_ERR_INVALID, "syn_pack_constants_host: buffer %zu < %zu bytes", bytes, need);
    std::vector<float> bb, bs;
    if (has_bb) arch_info(arch)->pack(arch, backbone_flat, bb);
    if (has_basis) pack_basis(w_shp, w_exp, u, param_mean, param_std, keypoints, n_lmk, n_vert, bs);
    ConstHeader hd{};
    hd.magic = kMagic; hd.version = kConstVersion;
    hd.has_backbone = has_bb; hd.has_basis = has_basis;
    if (has_basis) { hd.n_vert = n_vert; hd.n_lmk = n_lmk; hd.nvp = round_up(n_vert, 32); hd.nlp = round_up(n_lmk, 32); }
    hd.arch = has_bb ? arch : 0;
    hd.backbone_floats = bb.size(); hd.basis_floats = bs.size();
    hd.total_bytes = need;
    char *d = (char *)host_dst;
    memcpy(d, &hd, sizeof hd); d += sizeof hd;
    if (has_bb) { memcpy(d, bb.data(), bb.size() * sizeof(float)); d += bb.size() * sizeof(float); }
    if (has_basis) memcpy(d, bs.data(), bs.size() * sizeof(float));
    return SYN_OK;
}

namespace {
// the acceptance checks of a constants blob, on a host copy of its header; shared by the device import and the host twin
int check_const_header(const ConstHeader &hd, size_t bytes, const char *who) {
    if (hd.magic != kMagic) return fail(SYN_ERR_INVALID, "%s: bad magic", who);
    if (hd.version != kConstVersion) return fail(SYN_ERR_INVALID, "%s: constants blob version %u, this library packs version %u", who, hd.version, kConstVersion);
    if (hd.total_bytes > bytes) return fail(SYN_ERR_INVALID, "%s: header says %llu bytes, buffer has %zu", who,
                                            (unsigned long long)hd.total_bytes, bytes);
    if (hd.has_backbone && (!arch_known((int)hd.arch) || hd.backbone_floats != backbone_floats((int)hd.arch)))
        return fail(SYN_ERR_INVALID, "%s: backbone size mismatch", who);
    if (hd.has_basis && (hd.nvp % 32 || hd.nlp % 32 || hd.n_vert == 0 || hd.n_lmk == 0 || hd.n_vert > hd.nvp || hd.n_lmk > hd.nlp ||
                         hd.nvp - hd.n_vert >= 32 || hd.nlp - hd.n_lmk >= 32 || hd.basis_floats != basis_float_count(hd.nvp, hd.nlp)))
        return fail(SYN_ERR_INVALID, "%s: basis size mismatch", who);
    const uint64_t payload = sizeof(ConstHeader) + ((hd.has_backbone ? hd.backbone_floats : 0) + (hd.has_basis ? hd.basis_floats : 0)) * sizeof(float);
    if (payload > bytes || payload > hd.total_bytes)
        return fail(SYN_ERR_INVALID, "%s: header + payload = %llu bytes, buffer has %zu", who, (unsigned long long)payload, bytes);
    return SYN_OK;
}
}  // namespace

int syn_check_constants_host(const void *host_blob, size_t bytes) {
    if (!host_blob) return fail(SYN_ERR_INVALID, "syn_check_constants_host: NULL argument");
    if (bytes < sizeof(ConstHeader)) return fail(SYN_ERR_INVALID, "syn_check_constants_host: %zu bytes is smaller than the header", bytes);
    ConstHeader hd;
    memcpy(&hd, host_blob, sizeof hd);
    return check_const_header(hd, bytes, "syn_check_constants_host");
}

// ---- the broadcast itself, for a caller without torch.distributed (syn_bcast_constants(h, ncclComm_t, root, stream)) ----
// The communicator belongs to the caller's RCCL instance, so this library must call THAT instance: nothing is linked; the three entry
// points are resolved at the first call from what the process already holds (global scope, then librccl.so.1 as loaded by the caller
// or by torch -- RTLD_NOLOAD finds a library whatever scope it was loaded into), and only then from the ROCm installation.
namespace {
struct RcclApi {
    int (*Broadcast)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;       // ncclBroadcast
    int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;       // ncclAllReduce (the agreement steps: required, a rank without it would diverge)
    int (*CommUserRank)(void *, int *) = nullptr;                                                 // ncclCommUserRank
    const char *(*GetErrorString)(int) = nullptr;                                                 // ncclGetErrorString
    bool ok = false;
    bool explicit_failed = false;                                                                  // SYNERGY_HIP_RCCL_LIB was set and that instance is unusable
};
// SYNERGY_HIP_RCCL_LIB: the path of the RCCL instance that owns the caller's communicator, for a process that holds more than one
// (ADVICE r4); default: what the process already holds -- global scope, librccl.so.1 as loaded by the caller or by torch
// (RTLD_NOLOAD finds a library whatever scope it was loaded into) -- and only then the ROCm installation.
const RcclApi &rccl_api() {
    static const RcclApi api = [] {
        RcclApi a;
        const char *own = getenv("SYNERGY_HIP_RCCL_LIB");
        void *cands[5] = {own && *own ? dlopen(own, RTLD_LAZY | RTLD_GLOBAL) : nullptr, RTLD_DEFAULT, dlopen("librccl.so.1", RTLD_LAZY | RTLD_NOLOAD),
                          dlopen("librccl.so", RTLD_LAZY | RTLD_NOLOAD), nullptr};
        for (int i = (own && *own) ? 0 : 1; i < 5 && !a.ok; ++i) {
            void *lib = i < 4 ? cands[i] : dlopen("librccl.so.1", RTLD_LAZY | RTLD_GLOBAL);
            // an explicit instance is never silently replaced by another one: if it does not load, or lacks an entry point, there is no RCCL
            if (i == 0 && !lib) { a.explicit_failed = true; break; }
            if (i != 1 && !lib) continue;
            a.Broadcast = reinterpret_cast<decltype(a.Broadcast)>(dlsym(lib, "ncclBroadcast"));
            a.AllReduce = reinterpret_cast<decltype(a.AllReduce)>(dlsym(lib, "ncclAllReduce"));
            a.CommUserRank = reinterpret_cast<decltype(a.CommUserRank)>(dlsym(lib, "ncclCommUserRank"));
            a.GetErrorString = reinterpret_cast<decltype(a.GetErrorString)>(dlsym(lib, "ncclGetErrorString"));
            a.ok = a.Broadcast && a.AllReduce && a.CommUserRank && a.GetErrorString;
            if (i == 0) { a.explicit_failed = !a.ok; break; }
        }
        return a;
    }();
    return api;
}

// the pieces bcast_constants_protocol (bcast_protocol.h) is made of, on HIP memory and the caller's RCCL communicator
struct RcclBcastOps {
    syn_handle *h; void *comm; hipStream_t s; const RcclApi &R; int my_rank;
    unsigned long long *word_dev = nullptr;              // 256 bytes: the size word and the agreement word travel through device memory
    const char *transport_error = nullptr;
    int rank() const { return my_rank; }
    bool loaded() const { return h->d_backbone || h->d_basis; }
    uint64_t bytes() const { return (uint64_t)syn_constants_bytes(h); }
    void *alloc(uint64_t n) { void *p = nullptr; return hipMalloc(&p, n) == hipSuccess ? p : nullptr; }
    void release(void *p) { (void)hipFree(p); }
    int export_to(void *p, uint64_t n) { return syn_export_constants(h, p, n, s); }
    int import_from(void *p, uint64_t n) { return syn_import_constants(h, p, n, s); }
    int broadcast_word(syn::BcastWord *w, int root) {    // the size word lives on the HOST: staged through word_dev
        static_assert(sizeof(syn::BcastWord) <= 64, "the word is staged through the first 64 bytes of word_dev");
        if (hipMemcpyAsync(word_dev, w, sizeof *w, hipMemcpyHostToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) { transport_error = "staging a word"; return 1; }
        if (int e = R.Broadcast(word_dev, word_dev, sizeof *w, 1 /*ncclUint8*/, root, comm, s)) { transport_error = R.GetErrorString(e); return 1; }
        if (hipMemcpyAsync(w, word_dev, sizeof *w, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) { transport_error = "reading a word back"; return 1; }
        return 0;
    }
    int broadcast(void *buf, uint64_t n, int root) {     // the blob: device memory of alloc(), whatever its size
        if (int e = R.Broadcast(buf, buf, n, 1 /*ncclUint8*/, root, comm, s)) { transport_error = R.GetErrorString(e); return 1; }
        return 0;
    }
    int agree(int code) {                                // the most severe (most negative) code of all ranks; codes are <= 0
        // every rank ENTERS the all-reduce whatever happened to its own staging copy (a rank that returned here would hang the others);
        // a rank whose copy failed contributes whatever the word holds and returns at least SYN_ERR_HIP itself
        int v = -code;
        const bool staged = hipMemcpyAsync(word_dev + 8, &v, sizeof v, hipMemcpyHostToDevice, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
        if (!staged && !code) code = SYN_ERR_HIP;        // (what sits in the word is then stale: the rank's own verdict is at least this error)
        if (int e = R.AllReduce(word_dev + 8, word_dev + 8, 1, 2 /*ncclInt32*/, 2 /*ncclMax*/, comm, s)) { transport_error = R.GetErrorString(e); return code ? code : SYN_ERR_HIP; }
        if (hipMemcpyAsync(&v, word_dev + 8, sizeof v, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return code ? code : SYN_ERR_HIP;
        if (!staged) return code;
        return -v;
    }
};
}  // namespace

// A collective fails collectively (bcast_protocol.h): a root that has loaded nothing, or cannot stage its blob, says so IN the first
// broadcast and every rank returns that error together; a rank that cannot stage or import says so in an agreement step (all-reduce of the
// status) and every rank returns it.  The one failure that stays local is a rank that cannot allocate the 256-byte word buffer: it has no
// device memory to join a collective with.
int syn_bcast_constants(syn_handle *h, void *nccl_comm, int root, void *stream) {
    if (!h) return fail(SYN_ERR_INVALID, "syn_bcast_constants: NULL handle");
    if (!nccl_comm) return fail(SYN_ERR_INVALID, "syn_bcast_constants: NULL communicator");
    if (root < 0) return fail(SYN_ERR_INVALID, "syn_bcast_constants: root %d", root);
    const RcclApi &R = rccl_api();
    if (R.explicit_failed) return fail(SYN_ERR_NOT_LOADED, "syn_bcast_constants: SYNERGY_HIP_RCCL_LIB=%s cannot be loaded or lacks ncclBroadcast / ncclAllReduce / ncclCommUserRank / ncclGetErrorString (no other RCCL instance is tried in its place)", getenv("SYNERGY_HIP_RCCL_LIB"));
    if (!R.ok) return fail(SYN_ERR_NOT_LOADED, "syn_bcast_constants: no RCCL in this process (ncclBroadcast / ncclCommUserRank not found, librccl.so.1 not loadable; SYNERGY_HIP_RCCL_LIB names an instance explicitly)");
    DeviceGuard g(h->device);
    int rank = -1;
    if (int e = R.CommUserRank(nccl_comm, &rank)) return fail(SYN_ERR_HIP, "syn_bcast_constants: ncclCommUserRank: %s", R.GetErrorString(e));
    RcclBcastOps ops{h, nccl_comm, (hipStream_t)stream, R, rank};
    HIP_TRY(hipMalloc((void **)&ops.word_dev, 256));
    const char *where = "";
    const int rc = syn::bcast_constants_protocol(ops, root, SYN_ERR_NOT_LOADED, SYN_ERR_HIP, SYN_ERR_HIP, SYN_ERR_INVALID, &where);
    (void)hipFree(ops.word_dev);
    if (rc) return fail(rc, "syn_bcast_constants (rank %d, root %d): %s%s%s", rank, root, where, ops.transport_error ? ": " : "", ops.transport_error ? ops.transport_error : "");
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return fail(SYN_ERR_HIP, "syn_bcast_constants: stream synchronisation failed");
    return SYN_OK;
}

size_t syn_constants_bytes(syn_handle *h) {
    if (!h) return 0;
    return sizeof(ConstHeader) + ((h->d_backbone ? backbone_floats(h->arch) : 0) + (h->d_basis ? h->basis_floats : 0)) * sizeof(float);
}

static ConstHeader make_const_header(syn_handle *h) {
    ConstHeader hd{};
    hd.magic = kMagic; hd.version = kConstVersion;
    hd.has_backbone = h->d_backbone ? 1 : 0; hd.has_basis = h->d_basis ? 1 : 0;
    hd.n_vert = h->n_vert; hd.n_lmk = h->n_lmk; hd.nvp = h->nvp; hd.nlp = h->nlp;
    hd.arch = h->arch;
    hd.backbone_floats = hd.has_backbone ? backbone_floats(h->arch) : 0;
    hd.basis_floats = hd.has_basis ? h->basis_floats : 0;
    hd.total_bytes = syn_constants_bytes(h);
    return hd;
}

int syn_describe_constants(syn_handle *h, void *host_header, size_t bytes) {
    if (!h || !host_header) return fail(SYN_ERR_INVALID, "syn_describe_constants: NULL argument");
    if (bytes < sizeof(ConstHeader)) return fail(SYN_ERR_INVALID, "syn_describe_constants: %zu bytes is smaller than the header (%zu)", bytes, sizeof(ConstHeader));
    const ConstHeader hd = make_const_header(h);
    memcpy(host_header, &hd, sizeof hd);
    return SYN_OK;
}

int syn_export_constants(syn_handle *h, void *dev_dst, size_t bytes, void *stream) {
    if (!h || !dev_dst) return fail(SYN_ERR_INVALID, "syn_export_constants: NULL argument");
    const size_t need = syn_constants_bytes(h);
    if (bytes < need) return fail(SYN_ERR_INVALID, "syn_export_constants: buffer %zu < %zu bytes", bytes, need);
    ConstHeader hd = make_const_header(h);
    DeviceGuard g(h->device);
    hipStream_t s = (hipStream_t)stream;
    char *d = (char *)dev_dst;
    HIP_TRY(hipMemcpyAsync(d, &hd, sizeof hd, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));   // hd is a stack object
    d += sizeof hd;
    if (hd.has_backbone) {
        HIP_TRY(hipMemcpyAsync(d, h->d_backbone, hd.backbone_floats * sizeof(float), hipMemcpyDeviceToDevice, s));
        d += hd.backbone_floats * sizeof(float);
    }
    if (hd.has_basis) HIP_TRY(hipMemcpyAsync(d, h->d_basis, hd.basis_floats * sizeof(float), hipMemcpyDeviceToDevice, s));
    return SYN_OK;
}

int syn_import_constants(syn_handle *h, const void *dev_src, size_t bytes, void *stream) {
    if (!h || !dev_src) return fail(SYN_ERR_INVALID, "syn_import_constants: NULL argument");
    if (bytes < sizeof(ConstHeader)) return fail(SYN_ERR_INVALID, "syn_import_constants: %zu bytes is smaller than the header", bytes);
    DeviceGuard g(h->device);
    hipStream_t s = (hipStream_t)stream;
    ConstHeader hd{};
    HIP_TRY(hipMemcpyAsync(&hd, dev_src, sizeof hd, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (int rc = check_const_header(hd, bytes, "syn_import_constants")) return rc;
    const char *d = (const char *)dev_src + sizeof hd;
    if (hd.has_backbone) {
        if (h->d_backbone && h->arch != (int)hd.arch) { HIP_TRY(hipFree(h->d_backbone)); h->d_backbone = nullptr; }
        h->arch = (int)hd.arch;
        if (!h->d_backbone) HIP_TRY(hipMalloc((void **)&h->d_backbone, hd.backbone_floats * sizeof(float)));
        HIP_TRY(hipMemcpyAsync(h->d_backbone, d, hd.backbone_floats * sizeof(float), hipMemcpyDeviceToDevice, s));
        reset_backbone_state(h);
        if (h->arch == 0) {          // the sender's verdict on its weights rides in the blob
            HIP_TRY(hipMemcpyAsync(&h->ri, d + net().dst_range * sizeof(float), sizeof h->ri, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
        } else if (h->arch == 1) {
            HIP_TRY(hipMemcpyAsync(h->resnet_w_unsafe, d + resnet50().dst_range * sizeof(float), sizeof h->resnet_w_unsafe, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
        }
        d += hd.backbone_floats * sizeof(float);
    }
    if (hd.has_basis) {
        if (h->d_basis && h->basis_floats != hd.basis_floats) { HIP_TRY(hipFree(h->d_basis)); h->d_basis = nullptr; }
        if (!h->d_basis) HIP_TRY(hipMalloc((void **)&h->d_basis, hd.basis_floats * sizeof(float)));
        HIP_TRY(hipMemcpyAsync(h->d_basis, d, hd.basis_floats * sizeof(float), hipMemcpyDeviceToDevice, s));
        h->basis_floats = hd.basis_floats; h->n_vert = hd.n_vert; h->n_lmk = hd.n_lmk; h->nvp = hd.nvp; h->nlp = hd.nlp;
    }
    return SYN_OK;
}

size_t syn_workspace_bytes(syn_handle *, int B) {
    if (B <= 0) return 0;
    return ((size_t)B * (ws_floats_per_face() + syn::kRecFloatsPerFace) + 1024 + syn::kRecSlack) * sizeof(float);
}

// the forward of whatever the handle runs, on fp32 NCHW crops (img) or uint8 HWC crops (img8)
static int run_forward(syn_handle *h, const float *img, const uint8_t *img8, int B, float *param, float *pool, hipStream_t s) {
    DeviceGuard g(h->device);
    if (is_bb(h->arch)) return run_resnet_basic(h, img, img8, B, param, pool, s);
    if (is_rs(h->arch)) return run_resnest50(h, img, img8, B, param, pool, s);
    if (is_gn(h->arch)) return run_ghostnet(h, img, img8, B, param, pool, s);
    if (is_mb1(h->arch)) return run_mobilenet1(h, img, img8, B, param, pool, s);
    if (h->arch == 1) return run_resnet50(h, img, img8, B, param, pool, s);
    return run_backbone(h, img, img8, B, param, pool, s);
}

int syn_backbone_forward(syn_handle *h, const float *img, int B, float *param, float *pool, void *stream) {
    if (!h || !img || !param) return fail(SYN_ERR_INVALID, "syn_backbone_forward: NULL argument");
    if (B <= 0) return fail(SYN_ERR_INVALID, "syn_backbone_forward: B=%d", B);
    if (!h->d_backbone) return fail(SYN_ERR_NOT_LOADED, "syn_backbone_forward: backbone weights not loaded");
    return run_forward(h, img, nullptr, B, param, pool, (hipStream_t)stream);
}

int syn_backbone_forward_u8(syn_handle *h, const uint8_t *img, int B, float *param, float *pool, void *stream) {
    if (!h || !img || !param) return fail(SYN_ERR_INVALID, "syn_backbone_forward_u8: NULL argument");
    if (B <= 0) return fail(SYN_ERR_INVALID, "syn_backbone_forward_u8: B=%d", B);
    if (!h->d_backbone) return fail(SYN_ERR_NOT_LOADED, "syn_backbone_forward_u8: backbone weights not loaded");
    return run_forward(h, nullptr, img, B, param, pool, (hipStream_t)stream);
}

int syn_backbone_profile(syn_handle *h, const uint8_t *img_hwc, int B, int max_launches, int *feature_of_launch,
                         float *ms_of_launch, double *flops_of_launch) {
    if (!h || !img_hwc || B <= 0 || !feature_of_launch || !ms_of_launch || !flops_of_launch)
        return fail(SYN_ERR_INVALID, "syn_backbone_profile: bad argument");
    if (!h->d_backbone) return fail(SYN_ERR_NOT_LOADED, "syn_backbone_profile: backbone weights not loaded");
    DeviceGuard g(h->device);
    float *param = nullptr;
    HIP_TRY(hipMalloc((void **)&param, (size_t)B * 62 * sizeof(float)));
    std::vector<hipEvent_t> marks;
    std::vector<int> feats;
    if (is_mb1(h->arch) || is_gn(h->arch) || is_rs(h->arch) || is_bb(h->arch)) {      // feature_of_launch = the launch codes of mb1_launch_layer / gn_ / rs_ / bb_launch_block
        LaunchMarks lm(nullptr);
        int rc = is_bb(h->arch) ? run_resnet_basic(h, nullptr, img_hwc, B, param, nullptr, lm.s, &lm)
               : is_rs(h->arch) ? run_resnest50(h, nullptr, img_hwc, B, param, nullptr, lm.s, &lm)
               : is_gn(h->arch) ? run_ghostnet(h, nullptr, img_hwc, B, param, nullptr, lm.s, &lm)
                                : run_mobilenet1(h, nullptr, img_hwc, B, param, nullptr, lm.s, &lm);
        int count = 0;
        if (rc == SYN_OK) {
            HIP_TRY(hipDeviceSynchronize());
            for (size_t i = 1; i < lm.events.size() && count < max_launches; ++i, ++count) {
                float ms = 0.f;
                (void)hipEventElapsedTime(&ms, lm.events[i - 1], lm.events[i]);
                feature_of_launch[count] = lm.codes[i];
                ms_of_launch[count] = ms;
                flops_of_launch[count] = lm.flops[i] * B;
            }
        }
        (void)hipFree(param);
        return rc == SYN_OK ? count : rc;
    }
    int rc = run_backbone(h, nullptr, img_hwc, B, param, nullptr, nullptr, -1, nullptr, -1, nullptr, &marks, &feats);
    int count = 0;
    if (rc == SYN_OK) {
        HIP_TRY(hipDeviceSynchronize());
        const Net &n = net();
        for (size_t i = 1; i < marks.size() && count < max_launches; ++i, ++count) {
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, marks[i - 1], marks[i]);
            feature_of_launch[count] = feats[i];
            ms_of_launch[count] = ms;
            double fl = 0;       // algorithmic FLOPs of the layers this launch covers (no halo / padding work)
            if (feats[i] == 19) {
                fl = 2.0 * 1280 * 62 + 16.0 * 1280;
                bool has18 = false;
                for (size_t j = 1; j < feats.size(); ++j) has18 |= feats[j] == 18;
                if (!has18) fl += 2.0 * 320 * 1280 * 16;          // fused head: features.18 rides in this launch
            }
            else if (feats[i] >= 100) {                  // a chain launch: features first .. last = code / 100 .. code % 100
                for (const Layer &L : n.layers)
                    if (L.feature >= feats[i] / 100 && L.feature <= feats[i] % 100)
                        fl += 2.0 * (L.kind == DW ? 9.0 * L.cout : (double)L.cin * L.cout) * L.hout * L.hout;
            }
            else if (i == 1 && feats[i] == 1) { for (const Layer &L : n.layers) if (L.feature <= 1) fl += 2.0 * (L.kind == STEM ? 27.0 * 32 : L.kind == DW ? 9.0 * L.cout : (double)L.cin * L.cout) * L.hout * L.hout; }
            else {
                // a launch after a fused block covers the whole feature; per-layer launches cover one layer each
                int same = 0;
                for (size_t j = 1; j < feats.size(); ++j) same += feats[j] == feats[i];
                int seen = 0;
                for (size_t j = 1; j <= i; ++j) seen += feats[j] == feats[i];
                int idx = 0;
                for (const Layer &L : n.layers) {
                    if (L.feature != feats[i]) continue;
                    ++idx;
                    if (same > 1 && idx != seen) continue;
                    fl += 2.0 * (L.kind == STEM ? 27.0 * 32 : L.kind == DW ? 9.0 * L.cout : (double)L.cin * L.cout) * L.hout * L.hout;
                }
            }
            flops_of_launch[count] = fl * B;
        }
    }
    for (hipEvent_t e : marks) (void)hipEventDestroy(e);
    (void)hipFree(param);
    return rc == SYN_OK ? count : rc;
}

// One layer of the loaded MobileNetV1 on caller-supplied activations (include/synergy_hip.h): the launches are those of run_mobilenet1
// (mb1_launch_layer).  Everything is vetted before a device is touched; a per-layer block without aux keeps its depthwise output in the
// handle's workspace, where run_mobilenet1 keeps it.
int syn_mobilenet1_layer(syn_handle *h, int layer, int fused, const void *in, int in_u8, int B, size_t n_in, float *out, size_t n_out,
                         float *aux, size_t n_aux, void *stream) {
    if (!h || !in || !out) return fail(SYN_ERR_INVALID, "syn_mobilenet1_layer: NULL argument (handle, in and out are required)");
    if (!is_mb1(h->arch))
        return fail(SYN_ERR_INVALID, "syn_mobilenet1_layer: this handle runs %s, expected mobilenet_1, mobilenet_05 or mobilenet_2", arch_name(h->arch));
    if (layer < 0 || layer > 14) return fail(SYN_ERR_INVALID, "syn_mobilenet1_layer: layer=%d, expected 0 (stem), 1..13 (blocks) or 14 (pool + heads)", layer);
    if (int rc = check_hook_batch("syn_mobilenet1_layer", B, fused)) return rc;
    if (in_u8 && layer != 0) return fail(SYN_ERR_INVALID, "syn_mobilenet1_layer: in_u8 is set on layer %d, expected only on layer 0 (the stem)", layer);
    const bool block = layer >= 1 && layer <= 13;
    if (aux && layer == 0) return fail(SYN_ERR_INVALID, "syn_mobilenet1_layer: aux on layer 0, expected NULL (the stem has no second output)");
    if (aux && block && fused)
        return fail(SYN_ERR_INVALID, "syn_mobilenet1_layer: aux with fused=1 on layer %d, expected NULL (the fused launch keeps the depthwise output on chip)", layer);
    const Mb1Net &n = mb1net(h->arch);
    size_t f_in, f_out, f_aux;
    mb1_layer_counts(n, layer, &f_in, &f_out, &f_aux);
    if (n_in != f_in * B || n_out != f_out * B || (aux ? n_aux != f_aux * B : n_aux != 0))
        return fail(SYN_ERR_INVALID, "syn_mobilenet1_layer: layer %d of %s at B=%d expected n_in=%zu n_out=%zu n_aux=%zu, got %zu %zu %zu", layer,
                    arch_name(h->arch), B, f_in * B, f_out * B, aux ? f_aux * B : (size_t)0, n_in, n_out, n_aux);
    if (!h->d_backbone) return fail(SYN_ERR_NOT_LOADED, "syn_mobilenet1_layer: backbone weights not loaded");
    DeviceGuard g(h->device);
    float *second = aux;
    if (block && !fused && !aux) {
        int rc = ensure_ws(h, B);
        if (rc) return rc;
        second = h->ws + 2 * (size_t)B * n.buf_io;
    }
    mb1_launch_layer(n, h->d_backbone, layer, fused != 0, in_u8 ? nullptr : (const float *)in, in_u8 ? (const uint8_t *)in : nullptr, B, out,
                     second, (hipStream_t)stream, [](int, double) {});
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

// One block of the loaded GhostNet on caller-supplied activations (include/synergy_hip.h): the launches are those of run_ghostnet
// (gn_launch_block), the intermediates live in the handle's workspace where run_ghostnet keeps them.  Everything is vetted before a launch.
int syn_ghostnet_block(syn_handle *h, int block, int fused, const float *in, int B, size_t n_in, float *out, size_t n_out, float *aux,
                       size_t n_aux, void *stream) {
    if (!h || !in || !out) return fail(SYN_ERR_INVALID, "syn_ghostnet_block: NULL argument (handle, in and out are required)");
    if (!is_gn(h->arch)) return fail(SYN_ERR_INVALID, "syn_ghostnet_block: this handle runs %s, expected ghostnet", arch_name(h->arch));
    if (block < 0 || block > 18)
        return fail(SYN_ERR_INVALID, "syn_ghostnet_block: block=%d, expected 0..15 (bottlenecks), 16 (ConvBnAct), 17 (pool + conv_head + heads) or 18 (conv_stem)", block);
    if (int rc = check_hook_batch("syn_ghostnet_block", B, fused)) return rc;
    const GnNet &n = gnnet();
    size_t f_in, f_out, f_aux;
    if (block == 18) { f_in = 3 * 120 * 120; f_out = 3600 * (size_t)GnNet::kStem; f_aux = 0; }
    else if (block == 16) { f_in = 16 * 160; f_out = 16 * (size_t)GnNet::kLast; f_aux = 0; }
    else if (block == 17) { f_in = 16 * (size_t)GnNet::kLast; f_out = 62; f_aux = GnNet::kPool; }
    else {
        const GnBlock &b = n.blocks[block];
        f_in = (size_t)b.hin * b.hin * b.cin; f_out = (size_t)b.hout * b.hout * b.cout; f_aux = b.se ? b.mid : 0;
    }
    if (aux && !f_aux) return fail(SYN_ERR_INVALID, "syn_ghostnet_block: aux on block %d, expected NULL (no SE gate and no pool there)", block);
    if (n_in != f_in * B || n_out != f_out * B || (aux ? n_aux != f_aux * B : n_aux != 0))
        return fail(SYN_ERR_INVALID, "syn_ghostnet_block: block %d at B=%d expected n_in=%zu n_out=%zu n_aux=%zu, got %zu %zu %zu", block, B, f_in * B,
                    f_out * B, aux ? f_aux * B : (size_t)0, n_in, n_out, n_aux);
    if (!h->d_backbone) return fail(SYN_ERR_NOT_LOADED, "syn_ghostnet_block: backbone weights not loaded");
    DeviceGuard g(h->device);
    if (block == 18) {            // the stem needs no workspace; `fused` selects nothing here
        gn_launch_stem(n, h->d_backbone, in, nullptr, B, out, (hipStream_t)stream);
        HIP_TRY(hipGetLastError());
        return SYN_OK;
    }
    int rc = ensure_ws(h, B);
    if (rc) return rc;
    const GnWs w = gn_ws(n, h->ws + 2 * (size_t)B * n.buf_io, B);
    gn_launch_block(n, h->d_backbone, block, fused != 0, in, B, out, aux, w, (hipStream_t)stream, [](int, double) {});
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

// One block of the loaded ResNeSt-50 on caller-supplied activations (include/synergy_hip.h): the launches are those of run_resnest50
// (rs_launch_block), the intermediates live in the handle's workspace where run_resnest50 keeps them.  Everything is vetted before a launch.
int syn_resnest50_block(syn_handle *h, int block, int fused, const float *in, int B, size_t n_in, float *out, size_t n_out, float *aux,
                        size_t n_aux, void *stream) {
    if (!h || !in || !out) return fail(SYN_ERR_INVALID, "syn_resnest50_block: NULL argument (handle, in and out are required)");
    if (!is_rs(h->arch)) return fail(SYN_ERR_INVALID, "syn_resnest50_block: this handle runs %s, expected resnest50", arch_name(h->arch));
    if (block < 0 || block > 17) return fail(SYN_ERR_INVALID, "syn_resnest50_block: block=%d, expected 0 (stem + max pool), 1..16 (bottlenecks) or 17 (pool + heads)", block);
    if (int rc = check_hook_batch("syn_resnest50_block", B, fused)) return rc;
    const RsNet &n = rsnet();
    size_t f_in, f_out, f_aux;
    rs_block_counts(n, block, &f_in, &f_out, &f_aux);
    if (aux && !f_aux) return fail(SYN_ERR_INVALID, "syn_resnest50_block: aux on block %d, expected NULL (no attention and no pool there)", block);
    if (n_in != f_in * B || n_out != f_out * B || (aux ? n_aux != f_aux * B : n_aux != 0))
        return fail(SYN_ERR_INVALID, "syn_resnest50_block: block %d at B=%d expected n_in=%zu n_out=%zu n_aux=%zu, got %zu %zu %zu", block, B, f_in * B,
                    f_out * B, aux ? f_aux * B : (size_t)0, n_in, n_out, n_aux);
    if (!h->d_backbone) return fail(SYN_ERR_NOT_LOADED, "syn_resnest50_block: backbone weights not loaded");
    DeviceGuard g(h->device);
    int rc = ensure_ws(h, B);
    if (rc) return rc;
    rs_launch_block(n, h->d_backbone, block, fused != 0, in, nullptr, 1, B, out, aux, h->ws + 2 * (size_t)B * n.buf_io, (hipStream_t)stream, [](int, double) {});
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

// One block of the loaded resnet18 / resnet34 on caller-supplied activations (include/synergy_hip.h): the launches are those of
// run_resnet_basic (bb_launch_block), the intermediates live in the handle's workspace where run_resnet_basic keeps them.  Everything is
// vetted before a launch.
int syn_resnet_basic_block(syn_handle *h, int block, int fused, const float *in, int B, size_t n_in, float *out, size_t n_out, void *stream) {
    if (!h || !in || !out) return fail(SYN_ERR_INVALID, "syn_resnet_basic_block: NULL argument (handle, in and out are required)");
    if (!is_bb(h->arch)) return fail(SYN_ERR_INVALID, "syn_resnet_basic_block: this handle runs %s, expected resnet18 or resnet34", arch_name(h->arch));
    const BbNet &n = bbnet(h->arch);
    if (block < 0 || block > n.last())
        return fail(SYN_ERR_INVALID, "syn_resnet_basic_block: block=%d, expected 0 (stem + max pool), 1..%d (BasicBlocks) or %d (pool + heads)", block, n.last() - 1, n.last());
    if (int rc = check_hook_batch("syn_resnet_basic_block", B, fused)) return rc;
    size_t f_in, f_out;
    bb_block_counts(n, block, &f_in, &f_out);
    if (n_in != f_in * B || n_out != f_out * B)
        return fail(SYN_ERR_INVALID, "syn_resnet_basic_block: block %d at B=%d expected n_in=%zu n_out=%zu, got %zu %zu", block, B, f_in * B, f_out * B, n_in, n_out);
    if (!h->d_backbone) return fail(SYN_ERR_NOT_LOADED, "syn_resnet_basic_block: backbone weights not loaded");
    DeviceGuard g(h->device);
    int rc = ensure_ws(h, B);
    if (rc) return rc;
    bb_launch_block(n, h->d_backbone, block, fused != 0, in, nullptr, B, out, nullptr, h->ws + 2 * (size_t)B * n.buf_io, (hipStream_t)stream, [](int, double) {});
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

// Profiling hook, not part of include/synergy_hip.h: runs the backbone with the fused block of
// .features[feature] instrumented; out8 (host) = summed s_memtime ticks of wave 0 per stage
// {stage0, expand, barrier, depthwise, barrier, project, epilogue} and the workgroup count.
// out8: 8 counters as above + 24 more (row-marching kernels: busy cycles per wave id of the workgroup) = 32 values.
int syn_debug_profile_block(syn_handle *h, const float *img, int B, int feature, unsigned long long *out8) {
    if (!h || !img || !out8 || B <= 0) return fail(SYN_ERR_INVALID, "syn_debug_profile_block: bad argument");
    if (!h->d_backbone) return fail(SYN_ERR_NOT_LOADED, "syn_debug_profile_block: backbone weights not loaded");
    if (is_mb1(h->arch) || is_gn(h->arch) || is_rs(h->arch) || is_bb(h->arch)) return fail(SYN_ERR_INVALID, "syn_debug_profile_block: this handle runs %s", arch_name(h->arch));
    DeviceGuard g(h->device);
    unsigned long long *d = nullptr;
    HIP_TRY(hipMalloc((void **)&d, 32 * sizeof(unsigned long long)));
    HIP_TRY(hipMemset(d, 0, 32 * sizeof(unsigned long long)));
    float *param = nullptr;
    HIP_TRY(hipMalloc((void **)&param, (size_t)B * 62 * sizeof(float)));
    int rc = run_backbone(h, img, nullptr, B, param, nullptr, nullptr, -1, nullptr, feature, d);
    if (rc == SYN_OK) {
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(out8, d, 32 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    }
    (void)hipFree(d);
    (void)hipFree(param);
    return rc;
}

// Test hook, not part of include/synergy_hip.h: output of .features[feature] as NHWC [B,H,W,C].
int syn_debug_feature(syn_handle *h, const float *img, int B, int feature, float *out, void *stream) {
    if (!h || !img || !out || B <= 0 || feature < 0 || feature > 18) return fail(SYN_ERR_INVALID, "syn_debug_feature: bad argument");
    if (!h->d_backbone) return fail(SYN_ERR_NOT_LOADED, "syn_debug_feature: backbone weights not loaded");
    if (is_mb1(h->arch) || is_gn(h->arch) || is_rs(h->arch) || is_bb(h->arch)) return fail(SYN_ERR_INVALID, "syn_debug_feature: this handle runs %s", arch_name(h->arch));
    DeviceGuard g(h->device);
    return run_backbone(h, img, nullptr, B, nullptr, nullptr, (hipStream_t)stream, feature, out);
}

// .features[first] .. [last] of the loaded mobilenet_v2 on caller-supplied activations (include/synergy_hip.h): run_backbone itself, entered
// at `first` and left at `last`, so the launches are those the forward selects for this batch under the handle's schedule.  Everything is
// vetted before a device is touched.
int syn_mobilenet2_span(syn_handle *h, int first, int last, const void *in, int in_u8, int B, size_t n_in, float *out, size_t n_out,
                        float *aux, size_t n_aux, int *launch_tags, int max_tags, void *stream) {
    if (!h || !in || !out || !launch_tags)
        return fail(SYN_ERR_INVALID, "syn_mobilenet2_span: NULL argument (expected handle, in, out and launch_tags)");
    if (h->arch != 0) return fail(SYN_ERR_INVALID, "syn_mobilenet2_span: this handle runs %s, expected mobilenet_v2", arch_name(h->arch));
    if (first < 0 || first > 19 || last < 0 || last > 19 || first > last)
        return fail(SYN_ERR_INVALID, "syn_mobilenet2_span: first=%d last=%d, expected 0 <= first <= last <= 19", first, last);
    if (first == 1 || (first == 0 && last == 0))
        return fail(SYN_ERR_INVALID, "syn_mobilenet2_span: first=%d last=%d, expected first = 0 with last >= 1 (the stem and features.1 share a launch) or first >= 2", first, last);
    if (first == 19) return fail(SYN_ERR_INVALID, "syn_mobilenet2_span: first=19, expected first <= 18 (19 = pool and heads, reached as last = 19)");
    if (in_u8 && first != 0) return fail(SYN_ERR_INVALID, "syn_mobilenet2_span: in_u8 is set with first=%d, expected only with first = 0 (the crops)", first);
    if (aux && last != 19) return fail(SYN_ERR_INVALID, "syn_mobilenet2_span: aux with last=%d, expected NULL (only last = 19 has a second output, the pool)", last);
    if (B < 1 || B > 65536)          // the kernels index pixels and pixel x channel quads in 32-bit integers
        return fail(SYN_ERR_INVALID, "syn_mobilenet2_span: B=%d, expected 1 <= B <= 65536", B);
    const Net &n = net();
    size_t f_in = (size_t)3 * syn::kImg * syn::kImg, f_out = syn::kParam, n_layers = 0;
    for (const Layer &L : n.layers) {
        if (L.feature < first || L.feature > last) continue;
        if (!n_layers && first >= 2) f_in = (size_t)L.cin * L.hin * L.hin;
        if (last <= 18) f_out = (size_t)L.cout * L.hout * L.hout;
        ++n_layers;
    }
    const size_t f_aux = aux ? (size_t)syn::kPool : 0, need_tags = n_layers + (last == 19 ? 1 : 0);     // (one launch per layer: the most any schedule issues)
    if (n_in != f_in * B || n_out != f_out * B || n_aux != f_aux * B)
        return fail(SYN_ERR_INVALID, "syn_mobilenet2_span: features %d..%d at B=%d expected n_in=%zu n_out=%zu n_aux=%zu, got %zu %zu %zu", first, last, B,
                    f_in * B, f_out * B, f_aux * B, n_in, n_out, n_aux);
    if (max_tags < 0 || (size_t)max_tags < need_tags)
        return fail(SYN_ERR_INVALID, "syn_mobilenet2_span: max_tags=%d, expected >= %zu (the per-layer launch count of features %d..%d)", max_tags, need_tags, first, last);
    if (!h->d_backbone) return fail(SYN_ERR_NOT_LOADED, "syn_mobilenet2_span: backbone weights not loaded");
    DeviceGuard g(h->device);
    std::vector<int> tags;
    const bool whole = last == 19;
    const int rc = run_backbone(h, (first == 0 && !in_u8) ? (const float *)in : nullptr, (first == 0 && in_u8) ? (const uint8_t *)in : nullptr, B,
                                whole ? out : nullptr, whole ? aux : nullptr, (hipStream_t)stream, whole ? -1 : last, whole ? nullptr : out, -1, nullptr,
                                nullptr, nullptr, first, first >= 2 ? (const float *)in : nullptr, &tags);
    if (rc != SYN_OK) return rc;
    for (size_t i = 0; i < tags.size() && i < (size_t)max_tags; ++i) launch_tags[i] = tags[i];
    return (int)tags.size();
}

// Blocks first .. last of the loaded resnet50 on caller-supplied activations (include/synergy_hip.h): run_resnet50 itself, entered at `first`
// and left behind `last`, so the launches -- and the kernel variant of each, which the launchers report through syn::resnet_launch_sink --
// are those the forward selects for this batch under the handle's schedule.  Everything is vetted before a device is touched.
int syn_resnet50_span(syn_handle *h, int first, int last, const void *in, int in_u8, int B, size_t n_in, float *out, size_t n_out,
                      float *aux, size_t n_aux, int *launch_tags, int max_tags, void *stream) {
    if (!h || !in || !out || !launch_tags)
        return fail(SYN_ERR_INVALID, "syn_resnet50_span: NULL argument (expected handle, in, out and launch_tags)");
    if (h->arch != 1) return fail(SYN_ERR_INVALID, "syn_resnet50_span: this handle runs %s, expected resnet50", arch_name(h->arch));
    if (first < 0 || first > 17 || last < 0 || last > 17 || first > last)
        return fail(SYN_ERR_INVALID, "syn_resnet50_span: first=%d last=%d, expected 0 <= first <= last <= 17", first, last);
    if (in_u8 && first != 0) return fail(SYN_ERR_INVALID, "syn_resnet50_span: in_u8 is set with first=%d, expected only with first = 0 (the crops)", first);
    if (aux && (last == 0 || last == 16))
        return fail(SYN_ERR_INVALID, "syn_resnet50_span: aux with last=%d, expected NULL (no fused launch ends block 0 or 16; aux is the next conv1 for last = 1..15, the pool for last = 17)", last);
    if (B < 1 || B > 65536)          // the kernels index pixels in 32-bit integers
        return fail(SYN_ERR_INVALID, "syn_resnet50_span: B=%d, expected 1 <= B <= 65536", B);
    const ResNet50 &n = resnet50();
    size_t f_in = (size_t)3 * syn::kImg * syn::kImg, f_out = 62, f_aux = 0, need_tags = 0;
    if (first >= 1 && first <= 16) { const RConv &c = n.convs[n.blocks[first - 1].c1]; f_in = (size_t)c.hin * c.hin * c.cin; }
    if (first == 17) f_in = (size_t)16 * 2048;
    if (last == 0) f_out = (size_t)900 * 64;
    if (last >= 1 && last <= 16) { const RConv &c = n.convs[n.blocks[last - 1].c3]; f_out = (size_t)c.hout * c.hout * c.cout; }
    if (aux && last == 17) f_aux = 2048;
    if (aux && last >= 1 && last <= 15) { const RConv &c = n.convs[n.blocks[last].c1]; f_aux = (size_t)c.hout * c.hout * c.cout; }
    for (int k = first; k <= last; ++k) need_tags += k == 0 ? 2 : k == 17 ? 1 : n.blocks[k - 1].ds >= 0 ? 4 : 3;      // (one launch per layer: the most any schedule issues)
    if (n_in != f_in * B || n_out != f_out * B || n_aux != f_aux * B)
        return fail(SYN_ERR_INVALID, "syn_resnet50_span: blocks %d..%d at B=%d expected n_in=%zu n_out=%zu n_aux=%zu, got %zu %zu %zu", first, last, B,
                    f_in * B, f_out * B, f_aux * B, n_in, n_out, n_aux);
    if (max_tags < 0 || (size_t)max_tags < need_tags)
        return fail(SYN_ERR_INVALID, "syn_resnet50_span: max_tags=%d, expected >= %zu (the per-layer launch count of blocks %d..%d)", max_tags, need_tags, first, last);
    if (!h->d_backbone) return fail(SYN_ERR_NOT_LOADED, "syn_resnet50_span: backbone weights not loaded");
    DeviceGuard g(h->device);
    syn::LaunchSink sink;
    RSpan sp;
    sp.first = first; sp.last = last; sp.sink = &sink;
    if (first >= 1) sp.in = (const float *)in;
    if (last <= 16) { sp.out = out; sp.aux = aux; }
    syn::resnet_launch_sink = &sink;
    const int rc = run_resnet50(h, (first == 0 && !in_u8) ? (const float *)in : nullptr, (first == 0 && in_u8) ? (const uint8_t *)in : nullptr, B,
                                last == 17 ? out : nullptr, last == 17 ? aux : nullptr, (hipStream_t)stream, 62, &sp);
    syn::resnet_launch_sink = nullptr;
    if (rc != SYN_OK) return rc;
    for (int i = 0; i < sink.n && i < max_tags && i < 160; ++i) launch_tags[i] = sink.codes[i];
    return sink.n | (sp.aux_written ? SYN_SPAN_AUX_WRITTEN : 0);
}

// Test hook, not part of include/synergy_hip.h: the two converters of syn_resnet50_span alone.  to_pairs != 0: fp32 [M][C] -> the pair format,
// else back; C % 32 == 0; device pointers, in != out.
int syn_debug_resnet_pairs(const float *in, float *out, size_t M, int C, int to_pairs, void *stream) {
    if (!in || !out || in == out || M == 0 || C <= 0 || C % 32) return fail(SYN_ERR_INVALID, "syn_debug_resnet_pairs: bad argument (expected in != out, M > 0, C a multiple of 32)");
    if (to_pairs) syn::launch_pair_from_f32(in, out, M, C, (hipStream_t)stream);
    else syn::launch_f32_from_pair(in, out, M, C, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

// Calibration of the range verdict on the CALLER'S crops (include/synergy_hip.h): the load-time analysis proves the overflow side, but
// its underflow side rests on the interval bound being within 2^8 of the true activations.  Here every block output of the default
// schedule is held against the exact fp32-MFMA schedule of the same library on real data; the first block that differs by more than
// `tol` (relative to the tensor's maximum) is switched to the exact kernel -- in the handle AND in the verdict words of the packed
// constants, so replicas that import them follow -- and the comparison goes on behind it.  Returns the number of blocks switched.
int syn_backbone_calibrate(syn_handle *h, const uint8_t *crops_u8, int B, float tol, void *stream) {
    if (!h || !crops_u8) return fail(SYN_ERR_INVALID, "syn_backbone_calibrate: NULL argument");
    if (B <= 0 || B > 256) return fail(SYN_ERR_INVALID, "syn_backbone_calibrate: B=%d (1 .. 256 crops)", B);
    if (!(tol > 0.f)) return fail(SYN_ERR_INVALID, "syn_backbone_calibrate: tol=%g", (double)tol);
    if (!h->d_backbone) return fail(SYN_ERR_NOT_LOADED, "syn_backbone_calibrate: backbone weights not loaded");
    if (h->arch != 0) return 0;                          // ResNet-50 is guarded at run time (syn_backbone_range_status); MobileNetV1 is exact fp32
    DeviceGuard g(h->device);
    hipStream_t s = (hipStream_t)stream;
    const Net &n = net();
    const size_t cap = (size_t)B * 60 * 60 * 16;       // the largest block output (features.1)
    float *d_a = nullptr, *d_b = nullptr;
    HIP_TRY(hipMalloc((void **)&d_a, 2 * cap * sizeof(float)));
    d_b = d_a + cap;
    std::vector<float> ha(cap), hb(cap);
    const int fusion0 = h->fusion;
    int switched = 0, rc = SYN_OK;
    for (int f = 1; f <= 17 && rc == SYN_OK; ++f) {
        size_t count = 0;
        for (const Layer &L : n.layers) if (L.feature == f) count = (size_t)B * L.cout * L.hout * L.hout;      // (the block's last layer)
        const unsigned bit = f == 1 ? 1u : 1u << f;      // bit 0 = stem + features.1
        if ((h->ri.unsafe1 & bit) || count == 0 || count > cap) continue;      // already on the exact kernel
        h->fusion = 2;
        rc = run_backbone(h, nullptr, crops_u8, B, nullptr, nullptr, s, f, d_a);
        h->fusion = 1;
        if (rc == SYN_OK) rc = run_backbone(h, nullptr, crops_u8, B, nullptr, nullptr, s, f, d_b);
        h->fusion = fusion0;
        if (rc != SYN_OK) break;
        if (hipMemcpyAsync(ha.data(), d_a, count * sizeof(float), hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipMemcpyAsync(hb.data(), d_b, count * sizeof(float), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
            rc = fail(SYN_ERR_HIP, "syn_backbone_calibrate: reading features.%d back failed", f);
            break;
        }
        double worst = 0, mag = 0;
        bool finite = true;
        for (size_t i = 0; i < count; ++i) {
            finite = finite && std::isfinite(ha[i]) && std::isfinite(hb[i]);
            const double d = fabs((double)ha[i] - (double)hb[i]);
            worst = d > worst ? d : worst;
            mag = fabs((double)hb[i]) > mag ? fabs((double)hb[i]) : mag;
        }
        if (!finite || worst > (double)tol * (mag > 0 ? mag : 1.0)) {
            h->ri.unsafe1 |= bit; h->ri.unsafe16 |= bit;
            ++switched;
        }
    }
    (void)hipFree(d_a);
    if (rc != SYN_OK) return rc;
    if (switched) HIP_TRY(hipMemcpy(h->d_backbone + n.dst_range, &h->ri, sizeof h->ri, hipMemcpyHostToDevice));
    return switched;
}

// Test hook, not part of include/synergy_hip.h: fill every scratch buffer of the handle with `byte` (0xFF = NaNs), so a test
// can show that no result depends on what earlier calls (or the allocator) left in the workspace.
int syn_debug_poison_workspace(syn_handle *h, int B, int byte) {
    if (!h || B <= 0) return fail(SYN_ERR_INVALID, "syn_debug_poison_workspace: bad argument");
    DeviceGuard g(h->device);
    int rc = ensure_ws(h, B);
    if (rc) return rc;
    rc = ensure_rec(h, B);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemset(h->ws, byte, h->ws_bytes));
    HIP_TRY(hipMemset(h->rec, byte, h->rec_bytes));
    if (h->rws) HIP_TRY(hipMemset(h->rws, byte, h->rws_bytes));
    if (h->dws) HIP_TRY(hipMemset(h->dws, byte, h->dws_bytes));
    HIP_TRY(hipDeviceSynchronize());
    return SYN_OK;
}

int syn_crop_resize(syn_handle *h, const uint8_t *frame, int H, int W, const int *box, const int *xofs, const int16_t *xcoef,
                    const int *yofs, const int16_t *ycoef, uint8_t *out, int B, void *stream) {
    if (!h || !frame || !box || !xofs || !xcoef || !yofs || !ycoef || !out) return fail(SYN_ERR_INVALID, "syn_crop_resize: NULL argument");
    if (B <= 0 || H <= 0 || W <= 0) return fail(SYN_ERR_INVALID, "syn_crop_resize: B=%d H=%d W=%d", B, H, W);
    DeviceGuard g(h->device);
    syn::launch_crop_resize(frame, H, W, box, xofs, xcoef, yofs, ycoef, out, B, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

int syn_crop_resize_frames(syn_handle *h, const uint8_t *frames, const long long *frame_off, const int *frame_dim, const int *face_frame,
                           const int *box, const int *xofs, const int16_t *xcoef, const int *yofs, const int16_t *ycoef, uint8_t *out, int B,
                           void *stream) {
    if (!h || !frames || !frame_off || !frame_dim || !face_frame || !box || !xofs || !xcoef || !yofs || !ycoef || !out)
        return fail(SYN_ERR_INVALID, "syn_crop_resize_frames: NULL argument");
    if (B <= 0) return fail(SYN_ERR_INVALID, "syn_crop_resize_frames: B=%d", B);
    DeviceGuard g(h->device);
    syn::launch_crop_resize(frames, 0, 0, box, xofs, xcoef, yofs, ycoef, out, B, (hipStream_t)stream, frame_off, frame_dim, face_frame);
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

int syn_lanczos4_tables(syn_handle *h, const int *sides, int n, int *ofs, int16_t *coef, void *stream) {
    if (!h) return fail(SYN_ERR_INVALID, "syn_lanczos4_tables: NULL handle");
    if (n < 0) return fail(SYN_ERR_INVALID, "syn_lanczos4_tables: n=%d", n);
    if (n == 0) return SYN_OK;
    if (!sides || !ofs || !coef) return fail(SYN_ERR_INVALID, "syn_lanczos4_tables: NULL argument");
    DeviceGuard g(h->device);
    // the sides are the caller's own numbers (syn_face_tables derives and checks its sides itself): read them back and refuse a side
    // below 1 before anything is launched
    std::vector<int> host((size_t)n);
    HIP_TRY(hipMemcpyAsync(host.data(), sides, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    for (int i = 0; i < n; ++i)
        if (host[i] < 1) return fail(SYN_ERR_INVALID, "syn_lanczos4_tables: sides[%d]=%d (a crop side is at least 1)", i, host[i]);
    syn::launch_lanczos4_tables(sides, n, ofs, coef, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

int syn_face_tables(syn_handle *h, const float *dets, int n, float *roi, int *box, int *xofs, int16_t *xcoef, int *yofs, int16_t *ycoef,
                    int *status, void *stream) {
    if (!h) return fail(SYN_ERR_INVALID, "syn_face_tables: NULL handle");
    if (n < 0) return fail(SYN_ERR_INVALID, "syn_face_tables: n=%d", n);
    if (n == 0) return SYN_OK;
    if (!dets || !roi || !box || !xofs || !xcoef || !yofs || !ycoef || !status) return fail(SYN_ERR_INVALID, "syn_face_tables: NULL argument");
    DeviceGuard g(h->device);
    syn::launch_face_tables(dets, n, roi, box, xofs, xcoef, yofs, ycoef, status, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

int syn_compact_detections(syn_handle *h, const float *dets, const int *counts, const int *order, int N, int K, float thres, float *rows,
                           int *face_frame, int *frame_faces, void *stream) {
    if (!h) return fail(SYN_ERR_INVALID, "syn_compact_detections: NULL handle");
    if (N < 0 || K < 1 || (long long)N * K > 0x7fffffffll) return fail(SYN_ERR_INVALID, "syn_compact_detections: N=%d K=%d", N, K);
    if (N == 0) return SYN_OK;
    if (!dets || !counts || !rows || !face_frame || !frame_faces) return fail(SYN_ERR_INVALID, "syn_compact_detections: NULL argument");
    DeviceGuard g(h->device);
    syn::launch_compact_detections(dets, counts, order, N, K, thres, rows, face_frame, frame_faces, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

int syn_reconstruct_pitched(syn_handle *h, const float *param, int B, int param_len, int dense, int transform, const float *roi,
                            float *out, int row_pitch, int pad_writable, void *stream) {
    if (!h || !param || !out) return fail(SYN_ERR_INVALID, "syn_reconstruct: NULL argument");
    if (param_len != SYN_PARAM_DIM) return fail(SYN_ERR_PARAM_LEN, "length of params mismatch");
    if (B <= 0) return fail(SYN_ERR_INVALID, "syn_reconstruct: B=%d", B);
    if (!h->d_basis) return fail(SYN_ERR_NOT_LOADED, "syn_reconstruct: 3DMM basis not loaded");
    const int n = dense ? h->n_vert : h->n_lmk;
    if (row_pitch < n) return fail(SYN_ERR_INVALID, "syn_reconstruct: row_pitch=%d < %d columns", row_pitch, n);
    DeviceGuard g(h->device);
    int rc = ensure_rec(h, B);
    if (rc) return rc;
    float *rec = h->rec;
    hipStream_t s = (hipStream_t)stream;
    if (h->fusion >= 2)
        syn::launch_reconstruct_f16(param, basis_mean_cs(h), basis_std_cs(h), dense ? basis_f16_dense(h) : basis_f16_lmk(h), n, dense ? h->nvp : h->nlp,
                                   roi, transform, out, row_pitch, pad_writable, B, s, rec);
    else
        syn::launch_reconstruct(param, basis_mean(h), basis_std(h), dense ? basis_dense(h) : basis_lmk(h), n, dense ? h->nvp : h->nlp,
                                roi, transform, out, row_pitch, B, s, rec);
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

// Introspection (bench): the dense reconstruction into a pitched output with HIP events around its two kernels; synchronises.
// ms[0] = the per-face prologue (recon_prep_f16_kernel), ms[1] = the contraction + pose epilogue + mesh stores (recon_f16_kernel
// launches): the kernel whose roofline is HBM writes, B * 3 * n_vert * 4 bytes.
int syn_reconstruct_profile(syn_handle *h, const float *param, int B, const float *roi, float *out, int row_pitch, int pad_writable, float *ms2) {
    if (!h || !param || !out || !ms2) return fail(SYN_ERR_INVALID, "syn_reconstruct_profile: NULL argument");
    if (B <= 0 || !h->d_basis || row_pitch < h->n_vert) return fail(SYN_ERR_INVALID, "syn_reconstruct_profile: bad argument");
    if (h->fusion < 2) return fail(SYN_ERR_INVALID, "syn_reconstruct_profile: the fp16x2 schedule only");
    DeviceGuard g(h->device);
    int rc = ensure_rec(h, B);
    if (rc) return rc;
    hipEvent_t ev[3];
    for (auto &e : ev) HIP_TRY(hipEventCreate(&e));
    syn::launch_reconstruct_f16(param, basis_mean_cs(h), basis_std_cs(h), basis_f16_dense(h), h->n_vert, h->nvp, roi, 1, out, row_pitch, pad_writable, B,
                                nullptr, h->rec, ev);
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) { (void)hipEventElapsedTime(&ms2[0], ev[0], ev[1]); (void)hipEventElapsedTime(&ms2[1], ev[1], ev[2]); }
    for (auto &x : ev) (void)hipEventDestroy(x);
    if (e != hipSuccess) return fail(SYN_ERR_HIP, "syn_reconstruct_profile: %s", hipGetErrorString(e));
    return SYN_OK;
}

int syn_reconstruct(syn_handle *h, const float *param, int B, int param_len, int dense, int transform, const float *roi,
                    float *out, void *stream) {
    if (!h) return fail(SYN_ERR_INVALID, "syn_reconstruct: NULL argument");
    return syn_reconstruct_pitched(h, param, B, param_len, dense, transform, roi, out, dense ? h->n_vert : h->n_lmk, 0, stream);
}

// ---------------------------------------------------------------------------------------------
// Mesh consumers: Sim3DR.get_normal / RenderPipeline / Sim3DR.rasterize / cv2.addWeighted
// ---------------------------------------------------------------------------------------------
namespace {
int ensure_rws(syn_handle *h, size_t bytes) {
    if (bytes <= h->rws_bytes) return SYN_OK;
    if (h->rws) { HIP_TRY(hipDeviceSynchronize()); HIP_TRY(hipFree(h->rws)); h->rws = nullptr; h->rws_bytes = 0; }
    HIP_TRY(hipMalloc(&h->rws, bytes));
    h->rws_bytes = bytes;
    return SYN_OK;
}
size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
}  // namespace

namespace {
// Uploads a topology ([ntri,3], indices already validated) with the CSR of incident triangles per vertex in ascending triangle
// order, corner order inside a triangle: exactly the order in which the reference's sequential loop adds triangle normals to
// a vertex (rasterize_kernel.cpp:187-198)
int upload_topology(syn_handle *h, const int32_t *tri, int ntri, int nver, int **d_tri, int **d_adj_off, int **d_adj_tri) {
    std::vector<int> off(nver + 1, 0), adj(3 * (size_t)ntri);
    for (int i = 0; i < 3 * ntri; ++i) off[tri[i] + 1]++;
    for (int v = 0; v < nver; ++v) off[v + 1] += off[v];
    std::vector<int> cur(off.begin(), off.end() - 1);
    for (int t = 0; t < ntri; ++t)
        for (int j = 0; j < 3; ++j) adj[cur[tri[3 * t + j]]++] = t;
    if (*d_tri) { HIP_TRY(hipDeviceSynchronize()); (void)hipFree(*d_tri); (void)hipFree(*d_adj_off); (void)hipFree(*d_adj_tri); *d_tri = *d_adj_off = *d_adj_tri = nullptr; }
    HIP_TRY(hipMalloc((void **)d_tri, sizeof(int) * 3 * (size_t)ntri));
    HIP_TRY(hipMalloc((void **)d_adj_off, sizeof(int) * (nver + 1)));
    HIP_TRY(hipMalloc((void **)d_adj_tri, sizeof(int) * 3 * (size_t)ntri));
    HIP_TRY(hipMemcpy(*d_tri, tri, sizeof(int) * 3 * (size_t)ntri, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(*d_adj_off, off.data(), sizeof(int) * (nver + 1), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(*d_adj_tri, adj.data(), sizeof(int) * 3 * (size_t)ntri, hipMemcpyHostToDevice));
    return SYN_OK;
}
struct Topo { const int *tri, *adj_off, *adj_tri; int ntri, nver; };
// the topology syn_mesh_shade* / syn_rasterize work on (syn_select_topology); tri == nullptr: not loaded
int drop_tex_coords(syn_handle *h, int slot) {
    if (h->d_texc[slot]) { HIP_TRY(hipDeviceSynchronize()); (void)hipFree(h->d_texc[slot]); h->d_texc[slot] = nullptr; }
    h->texc_nver[slot] = h->texc_own_tri[slot] = 0;
    return SYN_OK;
}
Topo current_topo(const syn_handle *h) {
    if (h->topo_slot == 1) return Topo{h->k_tri, h->k_adj_off, h->k_adj_tri, h->k_ntri, h->n_keep};
    return Topo{h->d_tri, h->d_adj_off, h->d_adj_tri, h->ntri, h->tri_nver};
}
}  // namespace

int syn_load_triangles(syn_handle *h, const int32_t *tri, int ntri, int nver) {
    if (!h || !tri || ntri <= 0 || nver <= 0) return fail(SYN_ERR_INVALID, "syn_load_triangles: bad argument");
    if (ntri >= (1 << 24)) return fail(SYN_ERR_INVALID, "syn_load_triangles: ntri=%d exceeds the 24-bit z-key field", ntri);
    for (int i = 0; i < 3 * ntri; ++i)
        if (tri[i] < 0 || tri[i] >= nver) return fail(SYN_ERR_INVALID, "syn_load_triangles: tri[%d]=%d out of range", i, tri[i]);
    DeviceGuard g(h->device);
    int rc = drop_tex_coords(h, 0);
    if (rc) return rc;
    rc = upload_topology(h, tri, ntri, nver, &h->d_tri, &h->d_adj_off, &h->d_adj_tri);
    if (rc) { h->ntri = h->tri_nver = 0; return rc; }
    h->ntri = ntri; h->tri_nver = nver;
    h->tri_max[0] = *std::max_element(tri, tri + 3 * (size_t)ntri);
    h->topo_slot = 0;
    return SYN_OK;
}

int syn_load_uv_map(syn_handle *h, const int32_t *coord_u, const int32_t *coord_v, int nver, const int32_t *keep_ind, int n_keep,
                    const int32_t *tri_kept, int ntri_kept) {
    if (!h || !coord_u || !coord_v || !keep_ind || !tri_kept || nver <= 0 || n_keep <= 0 || ntri_kept <= 0)
        return fail(SYN_ERR_INVALID, "syn_load_uv_map: bad argument");
    if (ntri_kept >= (1 << 24)) return fail(SYN_ERR_INVALID, "syn_load_uv_map: ntri_kept=%d exceeds the 24-bit z-key field", ntri_kept);
    int mx[4] = {0, 0, 0, 0};
    for (int i = 0; i < nver; ++i) {
        if (coord_u[i] < 0 || coord_v[i] < 0) return fail(SYN_ERR_INVALID, "syn_load_uv_map: negative UV pixel (%d, %d) at vertex %d", coord_u[i], coord_v[i], i);
        mx[0] = std::max(mx[0], (int)coord_u[i]); mx[1] = std::max(mx[1], (int)coord_v[i]);
    }
    for (int k = 0; k < n_keep; ++k) {
        if (keep_ind[k] < 0 || keep_ind[k] >= nver) return fail(SYN_ERR_INVALID, "syn_load_uv_map: keep_ind[%d]=%d out of range", k, keep_ind[k]);
        mx[2] = std::max(mx[2], (int)coord_u[keep_ind[k]]); mx[3] = std::max(mx[3], (int)coord_v[keep_ind[k]]);
    }
    for (int i = 0; i < 3 * ntri_kept; ++i)
        if (tri_kept[i] < 0 || tri_kept[i] >= n_keep) return fail(SYN_ERR_INVALID, "syn_load_uv_map: tri_kept[%d]=%d out of range", i, tri_kept[i]);
    DeviceGuard g(h->device);
    if (int rc0 = drop_tex_coords(h, 1)) return rc0;
    if (h->d_uv) { HIP_TRY(hipDeviceSynchronize()); (void)hipFree(h->d_uv); h->d_uv = nullptr; }
    h->uv_nver = h->n_keep = h->k_ntri = 0;
    if (h->topo_slot == 1) h->topo_slot = 0;
    HIP_TRY(hipMalloc((void **)&h->d_uv, sizeof(int) * (2 * (size_t)nver + n_keep)));
    HIP_TRY(hipMemcpy(h->d_uv, coord_u, sizeof(int) * nver, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->d_uv + nver, coord_v, sizeof(int) * nver, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->d_uv + 2 * (size_t)nver, keep_ind, sizeof(int) * n_keep, hipMemcpyHostToDevice));
    int rc = upload_topology(h, tri_kept, ntri_kept, n_keep, &h->k_tri, &h->k_adj_off, &h->k_adj_tri);
    if (rc) return rc;
    h->uv_nver = nver; h->n_keep = n_keep; h->k_ntri = ntri_kept;
    h->tri_max[1] = *std::max_element(tri_kept, tri_kept + 3 * (size_t)ntri_kept);
    for (int i = 0; i < 4; ++i) h->uv_max[i] = mx[i];
    return SYN_OK;
}

int syn_select_topology(syn_handle *h, int slot) {
    if (!h || (slot != 0 && slot != 1)) return fail(SYN_ERR_INVALID, "syn_select_topology: slot must be 0 (syn_load_triangles) or 1 (syn_load_uv_map)");
    if (slot == 1 && !h->k_ntri) return fail(SYN_ERR_NOT_LOADED, "syn_select_topology: UV map not loaded");
    if (slot == 0 && !h->d_tri) return fail(SYN_ERR_NOT_LOADED, "syn_select_topology: triangles not loaded");
    h->topo_slot = slot;
    return SYN_OK;
}

int syn_uv_colors(syn_handle *h, const uint8_t *uv_tex, int T, int tex_h, int tex_w, int channels, int kept, int normalize, float *out,
                  void *stream) {
    if (!h || !uv_tex || !out) return fail(SYN_ERR_INVALID, "syn_uv_colors: NULL argument");
    if (T <= 0 || tex_h <= 0 || tex_w <= 0 || channels <= 0 || channels > 4)
        return fail(SYN_ERR_INVALID, "syn_uv_colors: T=%d tex_h=%d tex_w=%d channels=%d", T, tex_h, tex_w, channels);
    if (!h->d_uv || !h->uv_nver) return fail(SYN_ERR_NOT_LOADED, "syn_uv_colors: UV map not loaded");
    const int mu = h->uv_max[kept ? 2 : 0], mv = h->uv_max[kept ? 3 : 1];
    if (tex_h <= mu || tex_w <= mv)
        return fail(SYN_ERR_INVALID, "syn_uv_colors: a %d x %d texture is smaller than the UV table needs (%d x %d)", tex_h, tex_w, mu + 1, mv + 1);
    DeviceGuard g(h->device);
    syn::launch_uv_colors(uv_tex, h->d_uv, h->d_uv + h->uv_nver, kept ? h->d_uv + 2 * (size_t)h->uv_nver : nullptr, out, T,
                          kept ? h->n_keep : h->uv_nver, tex_h, tex_w, channels, normalize, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

int syn_gather_vertices(syn_handle *h, const float *vertices, int F, int planar, float *out, void *stream) {
    if (!h || !vertices || !out) return fail(SYN_ERR_INVALID, "syn_gather_vertices: NULL argument");
    if (F <= 0) return fail(SYN_ERR_INVALID, "syn_gather_vertices: F=%d", F);
    if (!h->d_uv || !h->n_keep) return fail(SYN_ERR_NOT_LOADED, "syn_gather_vertices: UV map not loaded");
    if (planar < 1 || (planar > 1 && planar < h->uv_nver))
        return fail(SYN_ERR_INVALID, "syn_gather_vertices: planar=%d (1 or a row pitch >= %d)", planar, h->uv_nver);
    if (planar == 1) planar = h->uv_nver;
    DeviceGuard g(h->device);
    syn::launch_gather_vertices(vertices, h->d_uv + 2 * (size_t)h->uv_nver, out, F, h->n_keep, planar, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

namespace {
int mesh_shade_impl(const char *who, syn_handle *h, const float *vertices, int F, int planar, const float *cfg16, float *normal,
                    float *light, float *tex, int shared, float *colors, void *stream) {
    const Topo T = current_topo(h);
    if (!T.tri) return fail(SYN_ERR_NOT_LOADED, "%s: triangles not loaded", who);
    if (planar < 0 || (planar > 1 && planar < T.nver)) return fail(SYN_ERR_INVALID, "%s: planar=%d (0, 1 or a row pitch >= %d)", who, planar, T.nver);
    if (planar == 1) planar = T.nver;
    DeviceGuard g(h->device);
    const size_t tn = align256(sizeof(float) * 3 * (size_t)T.ntri * F), mmb = align256(sizeof(unsigned) * 6 * F + 64);
    int rc = ensure_rws(h, tn + mmb);
    if (rc) return rc;
    float *tri_normal = (float *)h->rws;
    unsigned *mm = (unsigned *)((char *)h->rws + tn);
    float *d_cfg = (float *)(mm + 6 * F);            // 16 floats right behind the keys (inside the 64-byte tail)
    hipStream_t s = (hipStream_t)stream;
    syn::launch_mesh_normals(vertices, T.tri, T.adj_off, T.adj_tri, tri_normal, normal, mm, F, T.nver, T.ntri, planar, s);
    if (light || colors) {
        HIP_TRY(hipMemcpyAsync(d_cfg, cfg16, 16 * sizeof(float), hipMemcpyHostToDevice, s));
        if (colors) syn::launch_mesh_lighting_tex(vertices, normal, mm, d_cfg, light, tex, shared, colors, F, T.nver, planar, s);
        else syn::launch_mesh_lighting(vertices, normal, mm, d_cfg, light, F, T.nver, planar, s);
    }
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}
}  // namespace

int syn_mesh_shade(syn_handle *h, const float *vertices, int F, int planar, const float *cfg16, float *normal, float *light,
                   void *stream) {
    if (!h || !vertices || !normal) return fail(SYN_ERR_INVALID, "syn_mesh_shade: NULL argument");
    if (F <= 0) return fail(SYN_ERR_INVALID, "syn_mesh_shade: F=%d", F);
    if (light && !cfg16) return fail(SYN_ERR_INVALID, "syn_mesh_shade: light requested without a lighting configuration");
    return mesh_shade_impl("syn_mesh_shade", h, vertices, F, planar, cfg16, normal, light, nullptr, 0, nullptr, stream);
}

int syn_mesh_shade_textured(syn_handle *h, const float *vertices, int F, int planar, const float *cfg16, float *normal, float *light,
                            float *tex, int shared, float *colors, void *stream) {
    if (!h || !vertices || !normal || !cfg16 || !tex || !colors) return fail(SYN_ERR_INVALID, "syn_mesh_shade_textured: NULL argument");
    if (F <= 0) return fail(SYN_ERR_INVALID, "syn_mesh_shade_textured: F=%d", F);
    return mesh_shade_impl("syn_mesh_shade_textured", h, vertices, F, planar, cfg16, normal, light, tex, shared != 0, colors, stream);
}

int syn_rasterize(syn_handle *h, const float *vertices, const float *colors, int F, int planar, int channels, uint8_t *image,
                  int H, int W, int reverse, void *stream) {
    if (!h || !vertices || !colors || !image) return fail(SYN_ERR_INVALID, "syn_rasterize: NULL argument");
    if (F <= 0 || F > 254 || H <= 0 || W <= 0 || channels <= 0 || channels > 4)
        return fail(SYN_ERR_INVALID, "syn_rasterize: F=%d H=%d W=%d channels=%d", F, H, W, channels);
    const Topo T = current_topo(h);
    if (!T.tri) return fail(SYN_ERR_NOT_LOADED, "syn_rasterize: triangles not loaded");
    if (planar < 0 || (planar > 1 && planar < T.nver)) return fail(SYN_ERR_INVALID, "syn_rasterize: planar=%d (0, 1 or a row pitch >= %d)", planar, T.nver);
    if (planar == 1) planar = T.nver;
    DeviceGuard g(h->device);
    int rc = ensure_rws(h, sizeof(unsigned long long) * (size_t)H * W);
    if (rc) return rc;
    syn::launch_rasterize(vertices, T.tri, colors, (unsigned long long *)h->rws, image, F, T.nver, T.ntri, H, W, channels,
                          planar, reverse, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

int syn_rasterize_triangles(syn_handle *h, const float *vertices, int F, int planar, float *depth_buffer, int32_t *triangle_buffer,
                            float *barycentric_weight, int H, int W, void *stream) {
    if (!h || !vertices || !depth_buffer || !triangle_buffer || !barycentric_weight)
        return fail(SYN_ERR_INVALID, "syn_rasterize_triangles: NULL argument");
    if (F <= 0 || H <= 0 || W <= 0 || (long long)F * H * W >= (1ll << 31))
        return fail(SYN_ERR_INVALID, "syn_rasterize_triangles: F=%d H=%d W=%d (F*H*W must stay below 2^31)", F, H, W);
    const Topo T = current_topo(h);
    if (!T.tri) return fail(SYN_ERR_NOT_LOADED, "syn_rasterize_triangles: triangles not loaded");
    if (planar < 0 || (planar > 1 && planar < T.nver))
        return fail(SYN_ERR_INVALID, "syn_rasterize_triangles: planar=%d (0, 1 or a row pitch >= %d)", planar, T.nver);
    if (planar == 1) planar = T.nver;
    DeviceGuard g(h->device);
    int rc = ensure_rws(h, sizeof(unsigned long long) * (size_t)F * H * W);
    if (rc) return rc;
    syn::launch_rasterize_triangles(vertices, T.tri, (unsigned long long *)h->rws, depth_buffer, triangle_buffer, barycentric_weight, F,
                                    T.nver, T.ntri, H, W, planar, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

int syn_load_tex_coords(syn_handle *h, const float *tex_coords, int tex_nver, const int32_t *tex_triangles) {
    if (!h || !tex_coords || tex_nver <= 0) return fail(SYN_ERR_INVALID, "syn_load_tex_coords: bad argument");
    const int slot = h->topo_slot;
    const Topo tp = current_topo(h);
    const int ntri = tp.ntri;
    if (!tp.tri || !ntri) return fail(SYN_ERR_NOT_LOADED, "syn_load_tex_coords: triangles not loaded");
    if (h->tri_max[slot] >= tex_nver)                    // y is read through the MESH triangle's indices (rasterize_kernel.cpp:393-398)
        return fail(SYN_ERR_INVALID, "syn_load_tex_coords: the mesh triangles reach vertex %d, tex_nver=%d", h->tri_max[slot], tex_nver);
    for (int i = 0; tex_triangles && i < 3 * ntri; ++i)
        if (tex_triangles[i] < 0 || tex_triangles[i] >= tex_nver)
            return fail(SYN_ERR_INVALID, "syn_load_tex_coords: tex_triangles[%d]=%d out of range", i, tex_triangles[i]);
    DeviceGuard g(h->device);
    int rc = drop_tex_coords(h, slot);
    if (rc) return rc;
    const size_t fb = sizeof(float) * 3 * (size_t)tex_nver, tb = tex_triangles ? sizeof(int32_t) * 3 * (size_t)ntri : 0;
    HIP_TRY(hipMalloc((void **)&h->d_texc[slot], fb + tb));
    HIP_TRY(hipMemcpy(h->d_texc[slot], tex_coords, fb, hipMemcpyHostToDevice));
    if (tb) HIP_TRY(hipMemcpy((char *)h->d_texc[slot] + fb, tex_triangles, tb, hipMemcpyHostToDevice));
    h->texc_nver[slot] = tex_nver; h->texc_own_tri[slot] = tb != 0;
    return SYN_OK;
}

int syn_render_texture(syn_handle *h, const float *vertices, int F, int planar, const void *texture, int tex_u8, int T, int tex_h, int tex_w,
                       int tex_c, int mapping_type, void *image, int image_u8, float *depth_buffer, int H, int W, int c, int shared,
                       void *stream) {
    if (!h || !vertices || !texture || !image || !depth_buffer) return fail(SYN_ERR_INVALID, "syn_render_texture: NULL argument");
    if (F <= 0 || F > 65535 || H <= 0 || W <= 0 || (long long)F * H * W >= (1ll << 31))
        return fail(SYN_ERR_INVALID, "syn_render_texture: F=%d H=%d W=%d (F <= 65535, F*H*W must stay below 2^31)", F, H, W);
    if (c < 1 || c > 4 || tex_c > 4 || c > tex_c) return fail(SYN_ERR_INVALID, "syn_render_texture: c=%d tex_c=%d (1 <= c <= tex_c <= 4)", c, tex_c);
    if (T != 1 && T != F) return fail(SYN_ERR_INVALID, "syn_render_texture: T=%d textures for F=%d faces (1 or F)", T, F);
    if (mapping_type != 0 && mapping_type != 1) return fail(SYN_ERR_INVALID, "syn_render_texture: mapping_type=%d (0 nearest, 1 bilinear)", mapping_type);
    if (tex_h <= 0 || tex_w <= 0 || tex_h > (1 << 24) || tex_w > (1 << 24) || (long long)T * tex_h * tex_w >= (1ll << 31))
        return fail(SYN_ERR_INVALID, "syn_render_texture: T=%d tex_h=%d tex_w=%d (sides <= 2^24, T*tex_h*tex_w below 2^31)", T, tex_h, tex_w);
    const Topo tp = current_topo(h);
    if (!tp.tri) return fail(SYN_ERR_NOT_LOADED, "syn_render_texture: triangles not loaded");
    const int slot = h->topo_slot;
    if (!h->d_texc[slot]) return fail(SYN_ERR_NOT_LOADED, "syn_render_texture: texture coordinates not loaded (syn_load_tex_coords)");
    if ((unsigned long long)F * (unsigned long long)tp.ntri >= (1ull << 32))
        return fail(SYN_ERR_INVALID, "syn_render_texture: F=%d meshes of %d triangles exceed the 32-bit index field of the key", F, tp.ntri);
    if (planar < 0 || (planar > 1 && planar < tp.nver))
        return fail(SYN_ERR_INVALID, "syn_render_texture: planar=%d (0, 1 or a row pitch >= %d)", planar, tp.nver);
    if (planar == 1) planar = tp.nver;
    DeviceGuard g(h->device);
    int rc = ensure_rws(h, sizeof(unsigned long long) * (size_t)(shared ? 1 : F) * H * W);
    if (rc) return rc;
    const float *tc = h->d_texc[slot];
    const int *tex_tri = h->texc_own_tri[slot] ? (const int *)(tc + 3 * (size_t)h->texc_nver[slot]) : tp.tri;
    syn::launch_render_texture(vertices, tp.tri, tex_tri, tc, texture, tex_u8 != 0, T == F && F > 1, tex_h, tex_w, tex_c, mapping_type,
                               (unsigned long long *)h->rws, image, image_u8 != 0, depth_buffer, F, tp.nver, tp.ntri, H, W, c, planar,
                               shared != 0, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

int syn_vertex_visibility(syn_handle *h, const int32_t *triangle_buffer, int F, int H, int W, uint8_t *visible, void *stream) {
    if (!h || !triangle_buffer || !visible) return fail(SYN_ERR_INVALID, "syn_vertex_visibility: NULL argument");
    if (F <= 0 || H <= 0 || W <= 0 || (long long)F * H * W >= (1ll << 31))
        return fail(SYN_ERR_INVALID, "syn_vertex_visibility: F=%d H=%d W=%d (F*H*W must stay below 2^31)", F, H, W);
    const Topo T = current_topo(h);
    if (!T.tri) return fail(SYN_ERR_NOT_LOADED, "syn_vertex_visibility: triangles not loaded");
    DeviceGuard g(h->device);
    syn::launch_vertex_visibility(triangle_buffer, T.tri, visible, F, T.nver, T.ntri, H, W, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

int syn_sample_vertex_colors(syn_handle *h, const float *vertices, int F, int planar, const uint8_t *image, int H, int W, int channels,
                             int normalize, float *out, void *stream) {
    if (!h || !vertices || !image || !out) return fail(SYN_ERR_INVALID, "syn_sample_vertex_colors: NULL argument");
    if (F <= 0 || H <= 0 || W <= 0 || channels <= 0 || channels > 4 || (long long)H * W >= (1ll << 29))
        return fail(SYN_ERR_INVALID, "syn_sample_vertex_colors: F=%d H=%d W=%d channels=%d", F, H, W, channels);
    const Topo T = current_topo(h);
    if (!T.tri) return fail(SYN_ERR_NOT_LOADED, "syn_sample_vertex_colors: triangles not loaded");
    if (planar < 0 || (planar > 1 && planar < T.nver))
        return fail(SYN_ERR_INVALID, "syn_sample_vertex_colors: planar=%d (0, 1 or a row pitch >= %d)", planar, T.nver);
    if (planar == 1) planar = T.nver;
    DeviceGuard g(h->device);
    syn::launch_sample_vertex_colors(vertices, image, out, F, T.nver, H, W, channels, planar, normalize != 0, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

int syn_uv_scatter(syn_handle *h, const float *colors, const uint8_t *visible, int F, int channels, uint8_t *tex, uint8_t *mask, int tex_h,
                   int tex_w, void *stream) {
    if (!h || !colors || !tex || !mask) return fail(SYN_ERR_INVALID, "syn_uv_scatter: NULL argument");
    if (F <= 0 || tex_h <= 0 || tex_w <= 0 || channels <= 0 || channels > 4 || (long long)F * tex_h * tex_w >= (1ll << 29))
        return fail(SYN_ERR_INVALID, "syn_uv_scatter: F=%d tex_h=%d tex_w=%d channels=%d", F, tex_h, tex_w, channels);
    if (!h->d_uv || !h->uv_nver) return fail(SYN_ERR_NOT_LOADED, "syn_uv_scatter: UV map not loaded");
    if (tex_h <= h->uv_max[0] || tex_w <= h->uv_max[1])
        return fail(SYN_ERR_INVALID, "syn_uv_scatter: a %d x %d texture is smaller than the UV table needs (%d x %d)", tex_h, tex_w,
                    h->uv_max[0] + 1, h->uv_max[1] + 1);
    DeviceGuard g(h->device);
    int rc = ensure_rws(h, sizeof(unsigned) * (size_t)F * tex_h * tex_w);
    if (rc) return rc;
    syn::launch_uv_scatter(colors, visible, h->d_uv, h->d_uv + h->uv_nver, (unsigned *)h->rws, tex, mask, F, h->uv_nver, tex_h, tex_w,
                           channels, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

int syn_texture_fill(syn_handle *h, const uint8_t *tex_in, const uint8_t *mask, int T, int tex_h, int tex_w, int channels, int merge,
                     uint8_t *tex_out, void *stream) {
    if (!h || !tex_in || !mask || !tex_out) return fail(SYN_ERR_INVALID, "syn_texture_fill: NULL argument");
    if (T < 1 || tex_h < 1 || tex_h > syn::kTextureFillMaxDim || tex_w < 1 || tex_w > syn::kTextureFillMaxDim || channels < 1 || channels > 4)
        return fail(SYN_ERR_INVALID, "syn_texture_fill: T=%d tex_h=%d tex_w=%d channels=%d (T >= 1, sizes 1..4096, channels 1..4)", T, tex_h,
                    tex_w, channels);
    const size_t texels = (size_t)tex_h * tex_w;
    if (merge && (unsigned long long)T * texels > (1ull << 24))
        return fail(SYN_ERR_INVALID, "syn_texture_fill: merging T=%d views of %d x %d exceeds 2^24 texels, the sums would not fit 32 bits", T,
                    tex_h, tex_w);
    const int Tout = merge ? 1 : T;
    const unsigned long long tiles = (unsigned long long)Tout * ((tex_h + 63) / 64) * ((tex_w + 63) / 64);
    if (tiles >= (1ull << 31)) return fail(SYN_ERR_INVALID, "syn_texture_fill: T=%d textures of %d x %d are more tiles than one grid holds", T, tex_h, tex_w);
    const uint8_t *in_end = tex_in + (size_t)T * texels * channels, *out_end = tex_out + (size_t)Tout * texels * channels;
    if (tex_out < in_end && tex_in < out_end) return fail(SYN_ERR_INVALID, "syn_texture_fill: tex_out overlaps tex_in");
    if (tex_out < mask + (size_t)T * texels && mask < out_end) return fail(SYN_ERR_INVALID, "syn_texture_fill: tex_out overlaps mask");
    DeviceGuard g(h->device);
    int rc = ensure_rws(h, syn::texture_fill_scratch_bytes(Tout, tex_h, tex_w, channels));
    if (rc) return rc;
    syn::launch_texture_fill(tex_in, mask, (unsigned *)h->rws, tex_out, T, tex_h, tex_w, channels, merge != 0, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

int syn_add_weighted(syn_handle *h, const uint8_t *a, float alpha, const uint8_t *b, float beta, uint8_t *out, size_t n,
                     void *stream) {
    if (!h || !a || !b || !out) return fail(SYN_ERR_INVALID, "syn_add_weighted: NULL argument");
    DeviceGuard g(h->device);
    if (n) syn::launch_add_weighted(a, alpha, b, beta, out, n, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

// ---------------------------------------------------------------------------------------------
// FaceBoxes detector
// ---------------------------------------------------------------------------------------------
namespace {
struct DetConv { int cin, cout, k, stride, pad, kind; size_t src, w, shift; };     // kind: 0 crelu, 1 bn+relu, 2 head (bias)
struct DetNet {
    std::vector<DetConv> convs;
    size_t flat_count = 0, packed_count = 0;
    DetNet() {
        auto add = [&](int cin, int cout, int k, int st, int pad, int kind) {
            DetConv c{cin, cout, k, st, pad, kind, flat_count, packed_count, 0};
            flat_count += (size_t)cout * cin * k * k + (kind == 2 ? cout : 4 * cout);
            const int cp = round_up(cout, 4);
            packed_count += (size_t)k * k * cin * cp;
            c.shift = packed_count;
            packed_count += cp;
            convs.push_back(c);
        };
        add(3, 24, 7, 4, 3, 0); add(48, 64, 5, 2, 2, 0);                          // faceboxes.py:71-72
        for (int i = 0; i < 3; ++i) {                                              // Inception :21-30
            add(128, 32, 1, 1, 0, 1); add(128, 32, 1, 1, 0, 1); add(128, 24, 1, 1, 0, 1); add(24, 32, 3, 1, 1, 1);
            add(128, 24, 1, 1, 0, 1); add(24, 32, 3, 1, 1, 1); add(32, 32, 3, 1, 1, 1);
        }
        add(128, 128, 1, 1, 0, 1); add(128, 256, 3, 2, 1, 1); add(256, 128, 1, 1, 0, 1); add(128, 256, 3, 2, 1, 1);   // :78-82
        const int hc[3] = {128, 256, 256}, ha[3] = {21, 1, 1};
        for (int i = 0; i < 3; ++i) { add(hc[i], ha[i] * 4, 3, 1, 1, 2); add(hc[i], ha[i] * 2, 3, 1, 1, 2); }          // :104-114
    }
};
const DetNet &detnet() { static DetNet n; return n; }
int ensure_dws(syn_handle *h, size_t bytes) {
    if (bytes <= h->dws_bytes) return SYN_OK;
    if (h->dws) { HIP_TRY(hipDeviceSynchronize()); HIP_TRY(hipFree(h->dws)); h->dws = nullptr; h->dws_bytes = 0; }
    HIP_TRY(hipMalloc(&h->dws, bytes));
    h->dws_bytes = bytes;
    return SYN_OK;
}
int cdiv_i(int a, int b) { return (a + b - 1) / b; }
}  // namespace

size_t syn_detector_flat_count(void) { return detnet().flat_count; }

int syn_load_detector(syn_handle *h, const float *flat, size_t count) {
    if (!h || !flat) return fail(SYN_ERR_INVALID, "syn_load_detector: NULL argument");
    const DetNet &n = detnet();
    if (count != n.flat_count) return fail(SYN_ERR_INVALID, "syn_load_detector: %zu floats given, %zu expected", count, n.flat_count);
    std::vector<float> pk(n.packed_count, 0.f);
    for (const DetConv &c : n.convs) {
        const float *w = flat + c.src;
        const size_t wn = (size_t)c.cout * c.cin * c.k * c.k;
        const int cp = round_up(c.cout, 4);
        std::vector<float> sc(c.cout, 1.f), sh(c.cout, 0.f);
        if (c.kind == 2) { for (int o = 0; o < c.cout; ++o) sh[o] = w[wn + o]; }
        else {
            const float *g = w + wn, *b = g + c.cout, *m = b + c.cout, *v = m + c.cout;
            for (int o = 0; o < c.cout; ++o) { sc[o] = g[o] * (1.0f / sqrtf(v[o] + 1e-5f)); sh[o] = b[o] - m[o] * sc[o]; }
        }
        for (int o = 0; o < c.cout; ++o) {
            for (int ci = 0; ci < c.cin; ++ci)
                for (int ky = 0; ky < c.k; ++ky)
                    for (int kx = 0; kx < c.k; ++kx)
                        pk[c.w + ((size_t)(ky * c.k + kx) * c.cin + ci) * cp + o] = w[(((size_t)o * c.cin + ci) * c.k + ky) * c.k + kx] * sc[o];
            pk[c.shift + o] = sh[o];
        }
    }
    DeviceGuard g(h->device);
    if (!h->d_det) HIP_TRY(hipMalloc((void **)&h->d_det, n.packed_count * sizeof(float)));
    HIP_TRY(hipMemcpy(h->d_det, pk.data(), n.packed_count * sizeof(float), hipMemcpyHostToDevice));
    return SYN_OK;
}

// Enqueues the detector on N uint8 BGR frames of one size (device, contiguous).  scale: 1 or the down-scaling factor
// FaceBoxes.__call__ computes (FaceBoxes.py:63-80).  dets [N,keep_top_k,5] device; n_out [N] device, or nullptr for the slot in the
// workspace that *n_out_ws then points to (syn_detect downloads it).  Nothing synchronises unless the workspace has to grow.
// raw_loc / raw_conf / raw_boxes / raw_scores: optional device outputs of the network / decoder (tests, N = 1).
// `who`: the entry point's name for messages;  max_bytes: refuse a larger workspace (0 = no cap).
static int run_detect(syn_handle *h, const char *who, const uint8_t *frames, int N, int H, int W, int Hn, int Wn, float scale, float conf_thr,
                      float nms_thr, int top_k, int keep_top_k, float *dets, int *n_out, int **n_out_ws, size_t max_bytes, float *raw_loc,
                      float *raw_conf, float *raw_boxes, float *raw_scores, hipStream_t s) {
    const DetNet &n = detnet();
    if (Hn < 1 || Wn < 1) return fail(SYN_ERR_INVALID, "%s: scaled frame %dx%d", who, Hn, Wn);
    const int H1 = cdiv_i(Hn, 4), W1 = cdiv_i(Wn, 4), H2 = cdiv_i(H1, 2), W2 = cdiv_i(W1, 2), H3 = cdiv_i(H2, 2), W3 = cdiv_i(W2, 2);
    const int H4 = cdiv_i(H3, 2), W4 = cdiv_i(W3, 2), H5 = cdiv_i(H4, 2), W5 = cdiv_i(W4, 2), H6 = cdiv_i(H5, 2), W6 = cdiv_i(W5, 2);
    const int P = H4 * W4 * 21 + H5 * W5 + H6 * W6;
    // every prior can be a candidate; when more than the in-LDS sorter holds pass the threshold, the NMS kernel first selects
    // the top_k best of them exactly (radix select), which is all FaceBoxes.py:114-116 keeps
    const int max_cand = P;
    if (top_k > syn::det_sort_capacity())
        return fail(SYN_ERR_INVALID, "%s: top_k=%d exceeds the sorter's %d slots", who, top_k, syn::det_sort_capacity());
    // scratch carve (floats): the counters of all frames first, then one block of `fstride` floats per frame
    size_t off = 0;
    auto carve = [&](size_t nfl) { const size_t o = off; off += (nfl + 63) & ~(size_t)63; return o; };
    const size_t o_cnt = carve((size_t)N), o_nout = carve(64);
    const size_t head = off;
    const size_t o_img = carve((size_t)Hn * Wn * 3), o_c1 = carve((size_t)H1 * W1 * 48), o_p1 = carve((size_t)H2 * W2 * 48);
    const size_t o_c2 = carve((size_t)H3 * W3 * 128), o_xa = carve((size_t)H4 * W4 * 128), o_xb = carve((size_t)H4 * W4 * 128);
    const size_t o_pool = carve((size_t)H4 * W4 * 128), o_r1 = carve((size_t)H4 * W4 * 24), o_r2 = carve((size_t)H4 * W4 * 24);
    const size_t o_t = carve((size_t)H4 * W4 * 32), o_31 = carve((size_t)H4 * W4 * 128), o_32 = carve((size_t)H5 * W5 * 256);
    const size_t o_41 = carve((size_t)H5 * W5 * 128), o_42 = carve((size_t)H6 * W6 * 256);
    const size_t o_loc = carve((size_t)P * 4), o_conf = carve((size_t)P * 2), o_cand = carve((size_t)max_cand * 6);
    const size_t fstride = off - head;
    const size_t bytes = (head + fstride * (size_t)N) * sizeof(float);
    if (max_bytes && bytes > max_bytes)
        return fail(SYN_ERR_INVALID, "%s: N=%d frames of %dx%d need %zu bytes of scratch, more than the cap of %zu", who, N, Hn, Wn, bytes,
                    max_bytes);
    int rc = ensure_dws(h, bytes);
    if (rc) return rc;
    float *B0 = (float *)h->dws;
    const float *Wd = h->d_det;
    size_t li = 0;
    auto conv = [&](const float *in, int Hi, int Wi, int cs_in, int ci0, float *out, int Ho, int Wo, int cs_out, int co0) {
        const DetConv &c = n.convs[li++];
        syn::launch_det_conv(in, Wd + c.w, Wd + c.shift, out, N, fstride, Hi, Wi, cs_in, ci0, c.cin, Ho, Wo, cs_out, co0, c.cout, c.k, c.stride,
                             c.pad, c.kind == 0 ? 2 : (c.kind == 1 ? 1 : 0), s);
    };
    auto pool = [&](const float *in, float *out, int Hi, int Wi, int C, int Ho, int Wo, int stride, int is_max) {
        syn::launch_det_pool(in, out, N, fstride, Hi, Wi, C, Ho, Wo, stride, is_max, s);
    };
    syn::launch_det_preproc(frames, N, H, W, B0 + o_img, Hn, Wn, fstride, s);
    conv(B0 + o_img, Hn, Wn, 3, 0, B0 + o_c1, H1, W1, 48, 0);                                   // conv1 (CReLU -> 48)
    pool(B0 + o_c1, B0 + o_p1, H1, W1, 48, H2, W2, 2, 1);
    conv(B0 + o_p1, H2, W2, 48, 0, B0 + o_c2, H3, W3, 128, 0);                                  // conv2 (CReLU -> 128)
    pool(B0 + o_c2, B0 + o_xa, H3, W3, 128, H4, W4, 2, 1);
    float *x = B0 + o_xa, *y = B0 + o_xb;
    for (int i = 0; i < 3; ++i) {                                                               // Inception: cat[b1, b2, b3, b4]
        conv(x, H4, W4, 128, 0, y, H4, W4, 128, 0);                                             // branch1x1
        pool(x, B0 + o_pool, H4, W4, 128, H4, W4, 1, 0);
        conv(B0 + o_pool, H4, W4, 128, 0, y, H4, W4, 128, 32);                                  // branch1x1_2(avg_pool)
        conv(x, H4, W4, 128, 0, B0 + o_r1, H4, W4, 24, 0);                                      // branch3x3_reduce
        conv(B0 + o_r1, H4, W4, 24, 0, y, H4, W4, 128, 64);                                     // branch3x3
        conv(x, H4, W4, 128, 0, B0 + o_r2, H4, W4, 24, 0);                                      // branch3x3_reduce_2
        conv(B0 + o_r2, H4, W4, 24, 0, B0 + o_t, H4, W4, 32, 0);                                // branch3x3_2
        conv(B0 + o_t, H4, W4, 32, 0, y, H4, W4, 128, 96);                                      // branch3x3_3
        float *t2 = x; x = y; y = t2;
    }
    conv(x, H4, W4, 128, 0, B0 + o_31, H4, W4, 128, 0);
    conv(B0 + o_31, H4, W4, 128, 0, B0 + o_32, H5, W5, 256, 0);
    conv(B0 + o_32, H5, W5, 256, 0, B0 + o_41, H5, W5, 128, 0);
    conv(B0 + o_41, H5, W5, 128, 0, B0 + o_42, H6, W6, 256, 0);
    // multibox heads: NHWC conv outputs ARE the permuted / flattened loc and conf vectors (faceboxes.py:137-142)
    float *loc = B0 + o_loc, *conf = B0 + o_conf;
    const float *srcs[3] = {x, B0 + o_32, B0 + o_42};
    const int sh_[3] = {H4, H5, H6}, sw_[3] = {W4, W5, W6}, sc_[3] = {128, 256, 256}, sa[3] = {21, 1, 1};
    size_t lo = 0, co = 0;
    for (int i = 0; i < 3; ++i) {
        conv(srcs[i], sh_[i], sw_[i], sc_[i], 0, loc + lo, sh_[i], sw_[i], sa[i] * 4, 0);
        conv(srcs[i], sh_[i], sw_[i], sc_[i], 0, conf + co, sh_[i], sw_[i], sa[i] * 2, 0);
        lo += (size_t)sh_[i] * sw_[i] * sa[i] * 4; co += (size_t)sh_[i] * sw_[i] * sa[i] * 2;
    }
    int *cnt = (int *)(B0 + o_cnt);
    if (!n_out) n_out = (int *)(B0 + o_nout);
    if (n_out_ws) *n_out_ws = n_out;
    syn::launch_det_decode(loc, conf, N, fstride, P, Hn, Wn, H4, W4, H5, W5, H6, W6, scale, conf_thr, B0 + o_cand, cnt, max_cand, raw_boxes,
                           raw_scores, s);
    syn::launch_det_nms(B0 + o_cand, cnt, N, fstride, max_cand, top_k, nms_thr, keep_top_k, dets, n_out, s);
    if (raw_loc) HIP_TRY(hipMemcpyAsync(raw_loc, loc, sizeof(float) * 4 * P, hipMemcpyDeviceToDevice, s));
    if (raw_conf) HIP_TRY(hipMemcpyAsync(raw_conf, conf, sizeof(float) * 2 * P, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

// one frame, count returned to the host: the N = 1 case of the launches above + one 4-byte download and a stream synchronisation
static int run_detect_one(syn_handle *h, const uint8_t *frame, int H, int W, int Hn, int Wn, float scale, float conf_thr, float nms_thr,
                          int top_k, int keep_top_k, float *dets, int *n_dets, float *raw_loc, float *raw_conf, float *raw_boxes,
                          float *raw_scores, hipStream_t s) {
    int *d_n = nullptr;
    int rc = run_detect(h, "syn_detect", frame, 1, H, W, Hn, Wn, scale, conf_thr, nms_thr, top_k, keep_top_k, dets, nullptr, &d_n, 0, raw_loc,
                        raw_conf, raw_boxes, raw_scores, s);
    if (rc) return rc;
    int host_cnt = 0;
    HIP_TRY(hipMemcpyAsync(&host_cnt, d_n, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipGetLastError());
    *n_dets = host_cnt;
    return SYN_OK;
}

int syn_detector_prior_count(int Hn, int Wn) {
    return cdiv_i(Hn, 32) * cdiv_i(Wn, 32) * 21 + cdiv_i(Hn, 64) * cdiv_i(Wn, 64) + cdiv_i(Hn, 128) * cdiv_i(Wn, 128);
}

int syn_detect(syn_handle *h, const uint8_t *frame, int H, int W, int Hs, int Ws, float scale, float conf_thr, float nms_thr, int top_k,
               int keep_top_k, float *dets, int *n_dets, void *stream) {
    if (!h || !frame || !dets || !n_dets) return fail(SYN_ERR_INVALID, "syn_detect: NULL argument");
    if (H <= 0 || W <= 0 || Hs <= 0 || Ws <= 0 || Hs > H || Ws > W || !(scale > 0.f) || scale > 1.f || top_k <= 0 || keep_top_k <= 0)
        return fail(SYN_ERR_INVALID, "syn_detect: H=%d W=%d Hs=%d Ws=%d scale=%g top_k=%d keep_top_k=%d", H, W, Hs, Ws, (double)scale, top_k,
                    keep_top_k);
    if (!h->d_det) return fail(SYN_ERR_NOT_LOADED, "syn_detect: detector weights not loaded");
    DeviceGuard g(h->device);
    return run_detect_one(h, frame, H, W, Hs, Ws, scale, conf_thr, nms_thr, top_k, keep_top_k, dets, n_dets, nullptr, nullptr, nullptr, nullptr,
                          (hipStream_t)stream);
}

int syn_detect_batch(syn_handle *h, const uint8_t *frames, int N, int H, int W, int Hs, int Ws, float scale, float conf_thr, float nms_thr,
                     int top_k, int keep_top_k, float *dets, int *n_dets, void *stream) {
    if (!h || !frames || !dets || !n_dets) return fail(SYN_ERR_INVALID, "syn_detect_batch: NULL argument");
    if (N < 1 || N > SYN_DETECT_BATCH_MAX_FRAMES)
        return fail(SYN_ERR_INVALID, "syn_detect_batch: N=%d outside 1..%d", N, SYN_DETECT_BATCH_MAX_FRAMES);
    if (H <= 0 || W <= 0 || Hs <= 0 || Ws <= 0 || Hs > H || Ws > W || !(scale > 0.f) || scale > 1.f || top_k <= 0 || keep_top_k <= 0)
        return fail(SYN_ERR_INVALID, "syn_detect_batch: H=%d W=%d Hs=%d Ws=%d scale=%g top_k=%d keep_top_k=%d", H, W, Hs, Ws, (double)scale,
                    top_k, keep_top_k);
    if (!h->d_det) return fail(SYN_ERR_NOT_LOADED, "syn_detect_batch: detector weights not loaded");
    DeviceGuard g(h->device);
    return run_detect(h, "syn_detect_batch", frames, N, H, W, Hs, Ws, scale, conf_thr, nms_thr, top_k, keep_top_k, dets, n_dets, nullptr,
                      SYN_DETECT_BATCH_MAX_SCRATCH_BYTES, nullptr, nullptr, nullptr, nullptr, (hipStream_t)stream);
}

// Test hook, not part of include/synergy_hip.h: network outputs and decoded boxes / scores of every prior.
int syn_debug_detect_raw(syn_handle *h, const uint8_t *frame, int H, int W, int Hs, int Ws, float scale, float *loc, float *conf, float *boxes,
                         float *scores, void *stream) {
    if (!h || !frame || !h->d_det) return fail(SYN_ERR_INVALID, "syn_debug_detect_raw: bad argument");
    DeviceGuard g(h->device);
    float *dets = nullptr;
    HIP_TRY(hipMalloc((void **)&dets, 750 * 5 * sizeof(float)));
    int nd = 0;
    int rc = run_detect_one(h, frame, H, W, Hs, Ws, scale, 0.05f, 0.3f, 5000, 750, dets, &nd, loc, conf, boxes, scores, (hipStream_t)stream);
    (void)hipFree(dets);
    return rc;
}

// Test hook, not part of include/synergy_hip.h: det_nms_kernel alone, on candidate lists the caller made.  cand: device
// [N, max_cand, 6] float32 rows x1, y1, x2, y2, score, prior index (the bit pattern of a uint32), in any order -- the order of the
// atomic appends;  n_cand: device int [N], may exceed max_cand (clamped, as the decode kernel counts past a full list);
// dets: device [N, keep_top_k, 5];  n_dets: device int [N].  One launch on `stream`, no weights needed, no scratch.
int syn_debug_det_select_nms(syn_handle *h, const float *cand, const int *n_cand, int N, int max_cand, int top_k, float nms_thr,
                             int keep_top_k, float *dets, int *n_dets, void *stream) {
    if (!h || !cand || !n_cand || !dets || !n_dets) return fail(SYN_ERR_INVALID, "syn_debug_det_select_nms: NULL argument");
    if (N < 1 || max_cand < 1 || top_k <= 0 || keep_top_k <= 0)
        return fail(SYN_ERR_INVALID, "syn_debug_det_select_nms: N=%d max_cand=%d top_k=%d keep_top_k=%d", N, max_cand, top_k, keep_top_k);
    if (top_k > syn::det_sort_capacity())
        return fail(SYN_ERR_INVALID, "syn_debug_det_select_nms: top_k=%d exceeds the sorter's %d slots", top_k, syn::det_sort_capacity());
    DeviceGuard g(h->device);
    syn::launch_det_nms(cand, n_cand, N, (size_t)max_cand * 6, max_cand, top_k, nms_thr, keep_top_k, dets, n_dets, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

// Test hook, not part of include/synergy_hip.h: det_preproc_kernel alone.  frames: device uint8 [N,H,W,3] -> out: device float32
// [N,Hs,Ws,3] (Hs <= H, Ws <= W).
int syn_debug_det_preproc(syn_handle *h, const uint8_t *frames, int N, int H, int W, int Hs, int Ws, float *out, void *stream) {
    if (!h || !frames || !out) return fail(SYN_ERR_INVALID, "syn_debug_det_preproc: NULL argument");
    if (N < 1 || H <= 0 || W <= 0 || Hs <= 0 || Ws <= 0 || Hs > H || Ws > W)
        return fail(SYN_ERR_INVALID, "syn_debug_det_preproc: N=%d H=%d W=%d Hs=%d Ws=%d", N, H, W, Hs, Ws);
    DeviceGuard g(h->device);
    syn::launch_det_preproc(frames, N, H, W, out, Hs, Ws, (size_t)Hs * Ws * 3, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

int syn_nme(syn_handle *h, const float *fit, const float *gt, const float *roi, float *nme, int N, void *stream) {
    if (!h || !fit || !gt || !roi || !nme) return fail(SYN_ERR_INVALID, "syn_nme: NULL argument");
    if (N <= 0) return fail(SYN_ERR_INVALID, "syn_nme: N=%d", N);
    DeviceGuard g(h->device);
    syn::launch_nme(fit, gt, roi, nme, N, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

int syn_pose(syn_handle *h, const float *param, int B, const float *roi, double *angles, float *t3d, void *stream) {
    if (!h || !param || !angles || !t3d) return fail(SYN_ERR_INVALID, "syn_pose: NULL argument");
    if (B <= 0) return fail(SYN_ERR_INVALID, "syn_pose: B=%d", B);
    if (!h->d_basis) return fail(SYN_ERR_NOT_LOADED, "syn_pose: whitening statistics not loaded");
    DeviceGuard g(h->device);
    syn::launch_pose(param, basis_mean(h), basis_std(h), roi, angles, t3d, nullptr, B, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

int syn_landmarks_pose(syn_handle *h, const float *param, int B, int param_len, int transform, const float *roi, float *lmk, double *angles,
                       float *t3d, void *stream) {
    if (!h || !param || !lmk || !angles || !t3d) return fail(SYN_ERR_INVALID, "syn_landmarks_pose: NULL argument");
    if (param_len != SYN_PARAM_DIM) return fail(SYN_ERR_PARAM_LEN, "length of params mismatch");
    if (B <= 0) return fail(SYN_ERR_INVALID, "syn_landmarks_pose: B=%d", B);
    if (!h->d_basis) return fail(SYN_ERR_NOT_LOADED, "syn_landmarks_pose: 3DMM basis not loaded");
    DeviceGuard g(h->device);
    syn::launch_lmk_pose(param, basis_mean(h), basis_std(h), basis_lmk(h), h->n_lmk, h->nlp, roi, transform, lmk, angles, t3d, B, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

int syn_pose_matrix(syn_handle *h, const float *param, int B, float *pmat, void *stream) {
    if (!h || !param || !pmat) return fail(SYN_ERR_INVALID, "syn_pose_matrix: NULL argument");
    if (B <= 0) return fail(SYN_ERR_INVALID, "syn_pose_matrix: B=%d", B);
    if (!h->d_basis) return fail(SYN_ERR_NOT_LOADED, "syn_pose_matrix: whitening statistics not loaded");
    DeviceGuard g(h->device);
    syn::launch_pose(param, basis_mean(h), basis_std(h), nullptr, nullptr, nullptr, pmat, B, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// Synergy refinement: MLP_for / MLP_rev of backbone_nets/pointnet_backbone.py (include/synergy_hip.h; kernels: synergy_kernels.hip)
// ---------------------------------------------------------------------------------------------
namespace {
struct SynLayer { int cin, cout; };
const SynLayer kSynFor[9] = {{3, 64}, {64, 64}, {64, 64}, {64, 128}, {128, 1024}, {64 + syn::kSynFaceK, 512}, {512, 256}, {256, 128}, {128, 3}};
const SynLayer kSynRev[8] = {{3, 64}, {64, 64}, {64, 64}, {64, 128}, {128, 1024}, {1024, 12}, {1024, 40}, {1024, 10}};
size_t syn_mlp_count(const SynLayer *L, int n, int per_channel) {
    size_t c = 0;
    for (int i = 0; i < n; ++i) c += (size_t)L[i].cin * L[i].cout + (size_t)per_channel * L[i].cout;
    return c;
}
size_t synergy_flat_count() { return syn_mlp_count(kSynFor, 9, 5) + syn_mlp_count(kSynRev, 8, 5); }      // conv bias + 4 BatchNorm vectors
size_t synergy_folded_count() { return syn_mlp_count(kSynFor, 9, 2) + syn_mlp_count(kSynRev, 8, 2); }  // scale + shift

struct SynFolded { int cin = 0, cout = 0; std::vector<float> W, scale, shift; };
// one MLP of the flat layout: all convs (weight, bias), then all BatchNorms (gamma, beta, mean, var); eval BatchNorm1d, eps 1e-5
std::vector<SynFolded> fold_mlp(const float *flat, const SynLayer *L, int n) {
    std::vector<SynFolded> out(n);
    const float *conv = flat, *bn = flat + syn_mlp_count(L, n, 1);
    for (int i = 0; i < n; ++i) {
        SynFolded &f = out[i];
        f.cin = L[i].cin; f.cout = L[i].cout;
        const size_t nw = (size_t)f.cin * f.cout;
        f.W.assign(conv, conv + nw);
        const float *bias = conv + nw, *gamma = bn, *beta = bn + f.cout, *mean = bn + 2 * f.cout, *var = bn + 3 * f.cout;
        f.scale.resize(f.cout); f.shift.resize(f.cout);
        for (int c = 0; c < f.cout; ++c) {
            const double sc = (double)gamma[c] / std::sqrt((double)var[c] + 1e-5);
            f.scale[c] = (float)sc;
            f.shift[c] = (float)(((double)bias[c] - (double)mean[c]) * sc + (double)beta[c]);
        }
        conv += nw + f.cout;
        bn += 4 * (size_t)f.cout;
    }
    return out;
}
// MLP_rev's three heads as one [62][1024] layer: ori 12 | shape 40 | expr 10
SynFolded merge_rev_heads(const std::vector<SynFolded> &r) {
    SynFolded m;
    m.cin = 1024;
    for (int i = 5; i < 8; ++i) {
        m.cout += r[i].cout;
        m.W.insert(m.W.end(), r[i].W.begin(), r[i].W.end());
        m.scale.insert(m.scale.end(), r[i].scale.begin(), r[i].scale.end());
        m.shift.insert(m.shift.end(), r[i].shift.begin(), r[i].shift.end());
    }
    return m;
}
// columns [c0, c1) of a layer's weights
std::vector<float> weight_columns(const SynFolded &f, int c0, int c1) {
    std::vector<float> w((size_t)f.cout * (c1 - c0));
    for (int n = 0; n < f.cout; ++n)
        for (int k = c0; k < c1; ++k) w[(size_t)n * (c1 - c0) + (k - c0)] = f.W[(size_t)n * f.cin + k];
    return w;
}

// kernel-ready image: every matrix row-major [rows_pad][cols_pad] zero padded, every vector zero padded to rows_pad
struct SynBlob {
    std::vector<float> v;
    size_t matrix(const std::vector<float> &W, int rows, int cols, int rows_pad, int cols_pad) {
        const size_t at = v.size();
        v.resize(at + (size_t)rows_pad * cols_pad, 0.f);
        for (int r = 0; r < rows; ++r)
            for (int c = 0; c < cols; ++c) v[at + (size_t)r * cols_pad + c] = W[(size_t)r * cols + c];
        return at;
    }
    size_t vector(const std::vector<float> &x, int n_pad) {
        const size_t at = v.size();
        v.resize(at + n_pad, 0.f);
        for (size_t i = 0; i < x.size(); ++i) v[at + i] = x[i];
        return at;
    }
};
int pad16(int x) { return (x + 15) / 16 * 16; }

// Behind the sws_bytes of scratch lies a tail that no entry point uses as scratch: the ticket counter of the loss kernels
// (loss_kernels.hip), zeroed here and left at zero by every launch that uses it.
constexpr size_t kSwsTail = 256;
int ensure_sws(syn_handle *h, size_t bytes) {
    if (bytes <= h->sws_bytes) return SYN_OK;
    bytes = (bytes + 255) / 256 * 256;
    if (h->sws) { HIP_TRY(hipDeviceSynchronize()); HIP_TRY(hipFree(h->sws)); h->sws = nullptr; h->sws_bytes = 0; }
    HIP_TRY(hipMalloc(&h->sws, bytes + kSwsTail));
    HIP_TRY(hipMemset((char *)h->sws + bytes, 0, kSwsTail));
    HIP_TRY(hipDeviceSynchronize());
    h->sws_bytes = bytes;
    return SYN_OK;
}
unsigned *loss_counter(const syn_handle *h) { return (unsigned *)((char *)h->sws + h->sws_bytes); }
// scratch of a B-face call (floats): Lc [B,3,68] | pf [B*68,64] | X6 [B,2368] | g6 [B,512] | gf [B,1024]
constexpr size_t kSwsLc = 3 * syn::kSynPts, kSwsPf = 64 * syn::kSynPts, kSwsX6 = syn::kSynFaceKpad, kSwsG6 = 512, kSwsGf = syn::kSynGlobal;
constexpr size_t kSwsPerFace = kSwsLc + kSwsPf + kSwsX6 + kSwsG6 + kSwsGf;

syn::SynTrunkW trunk_weights(const syn_handle *h, int which) {
    syn::SynTrunkW w;
    for (int i = 0; i < 5; ++i) {
        w.W[i] = h->d_syn + h->syn_off.tW[which][i];
        w.scale[i] = h->d_syn + h->syn_off.tscale[which][i];
        w.shift[i] = h->d_syn + h->syn_off.tshift[which][i];
    }
    return w;
}

int synergy_ready(const syn_handle *h, const char *who) {
    if (h->arch != 0 && !is_gn(h->arch))          // ghostnet's pooled feature (the 1280 outputs of conv_head + ReLU) has the same width
        return fail(SYN_ERR_INVALID, "%s: the synergy refinement needs the 1280-d pooled feature of mobilenet_v2 or ghostnet; this handle runs %s (%d-d)", who,
                    arch_name(h->arch), arch_info(h->arch)->pool);
    if (!h->d_syn) return fail(SYN_ERR_NOT_LOADED, "%s: synergy weights not loaded (syn_load_synergy)", who);
    return SYN_OK;
}

// MLP_for on crop-space landmarks `lmk` (device) -> out = (lmk + 0.05 res), ROI affine if roi
int run_refine(syn_handle *h, const float *lmk, const float *pool, const float *param, int B, const float *roi, float *out, float *global_feat,
               hipStream_t s) {
    float *pf = h->sws + kSwsLc * B, *X6 = pf + kSwsPf * B, *g6 = X6 + kSwsX6 * B;
    const SynOffsets &o = h->syn_off;
    const float *d = h->d_syn;
    syn::launch_syn_trunk(trunk_weights(h, 0), lmk, B, pf, X6, syn::kSynFaceKpad, global_feat, s);
    syn::launch_syn_face_concat(pool, param, X6, B, s);
    syn::launch_syn_face_gemm(X6, syn::kSynFaceKpad, d + o.W6f, syn::kSynFaceKpad, nullptr, nullptr, g6, 512, 512, B, s);
    const syn::SynHeadW hw = {d + o.W6p, d + o.scale6, d + o.shift6, d + o.W7, d + o.scale7, d + o.shift7,
                              d + o.W8, d + o.scale8, d + o.shift8, d + o.W9, d + o.scale9, d + o.shift9};
    syn::launch_syn_point_head(hw, pf, g6, lmk, roi, out, B, s);
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}
bool overlap(const float *a, const float *b, size_t n) { return a < b + n && b < a + n; }
}  // namespace

extern "C" {

size_t syn_synergy_flat_count(void) { return synergy_flat_count(); }
size_t syn_synergy_folded_count(void) { return synergy_folded_count(); }

int syn_fold_synergy_host(const float *flat, size_t n, float *folded, size_t n_folded) {
    if (!flat || !folded) return fail(SYN_ERR_INVALID, "syn_fold_synergy_host: NULL argument");
    if (n != synergy_flat_count() || n_folded != synergy_folded_count())
        return fail(SYN_ERR_INVALID, "syn_fold_synergy_host: %zu / %zu floats, expected %zu / %zu", n, n_folded, synergy_flat_count(), synergy_folded_count());
    const std::vector<SynFolded> f = fold_mlp(flat, kSynFor, 9), r = fold_mlp(flat + syn_mlp_count(kSynFor, 9, 5), kSynRev, 8);
    float *p = folded;
    auto put = [&p](const std::vector<float> &x) { p = std::copy(x.begin(), x.end(), p); };
    auto layer = [&put](const SynFolded &L) { put(L.W); put(L.scale); put(L.shift); };
    for (int i = 0; i < 5; ++i) layer(f[i]);
    put(weight_columns(f[5], 0, 64));
    put(weight_columns(f[5], 64, f[5].cin));
    put(f[5].scale); put(f[5].shift);
    for (int i = 6; i < 9; ++i) layer(f[i]);
    for (int i = 0; i < 5; ++i) layer(r[i]);
    layer(merge_rev_heads(r));
    if ((size_t)(p - folded) != n_folded) return fail(SYN_ERR_INVALID, "syn_fold_synergy_host: internal layout mismatch");
    return SYN_OK;
}

int syn_load_synergy(syn_handle *h, const float *flat, size_t n) {
    if (!h || !flat) return fail(SYN_ERR_INVALID, "syn_load_synergy: NULL argument");
    if (n != synergy_flat_count()) return fail(SYN_ERR_INVALID, "syn_load_synergy: %zu floats, expected %zu", n, synergy_flat_count());
    if (syn::syn_flat_total() != synergy_flat_count()) return fail(SYN_ERR_INVALID, "syn_load_synergy: internal layout mismatch");
    const std::vector<SynFolded> f = fold_mlp(flat, kSynFor, 9), r = fold_mlp(flat + syn_mlp_count(kSynFor, 9, 5), kSynRev, 8);
    SynBlob b;
    SynOffsets o = {};
    for (int which = 0; which < 2; ++which) {
        const std::vector<SynFolded> &m = which ? r : f;
        for (int i = 0; i < 5; ++i) {
            o.tW[which][i] = b.matrix(m[i].W, m[i].cout, m[i].cin, m[i].cout, i == 0 ? 4 : m[i].cin);     // conv1: K = 3 -> 4 (one MFMA step)
            o.tscale[which][i] = b.vector(m[i].scale, m[i].cout);
            o.tshift[which][i] = b.vector(m[i].shift, m[i].cout);
        }
    }
    o.W6p = b.matrix(weight_columns(f[5], 0, 64), 512, 64, 512, 64);
    o.W6f = b.matrix(weight_columns(f[5], 64, f[5].cin), 512, syn::kSynFaceK, 512, syn::kSynFaceKpad);
    o.scale6 = b.vector(f[5].scale, 512); o.shift6 = b.vector(f[5].shift, 512);
    o.W7 = b.matrix(f[6].W, 256, 512, 256, 512); o.scale7 = b.vector(f[6].scale, 256); o.shift7 = b.vector(f[6].shift, 256);
    o.W8 = b.matrix(f[7].W, 128, 256, 128, 256); o.scale8 = b.vector(f[7].scale, 128); o.shift8 = b.vector(f[7].shift, 128);
    o.W9 = b.matrix(f[8].W, 3, 128, 16, 128); o.scale9 = b.vector(f[8].scale, 16); o.shift9 = b.vector(f[8].shift, 16);
    const SynFolded hd = merge_rev_heads(r);
    o.Wrev = b.matrix(hd.W, hd.cout, 1024, pad16(hd.cout), 1024);
    o.scale_rev = b.vector(hd.scale, pad16(hd.cout)); o.shift_rev = b.vector(hd.shift, pad16(hd.cout));
    DeviceGuard g(h->device);
    if (h->d_syn) { HIP_TRY(hipDeviceSynchronize()); HIP_TRY(hipFree(h->d_syn)); h->d_syn = nullptr; }     // replacing: nothing may still read the old weights
    HIP_TRY(hipMalloc(&h->d_syn, b.v.size() * sizeof(float)));
    HIP_TRY(hipMemcpy(h->d_syn, b.v.data(), b.v.size() * sizeof(float), hipMemcpyHostToDevice));
    if (!h->d_syn_flat) HIP_TRY(hipMalloc(&h->d_syn_flat, n * sizeof(float)));
    HIP_TRY(hipMemcpy(h->d_syn_flat, flat, n * sizeof(float), hipMemcpyHostToDevice));
    h->syn_off = o;
    return SYN_OK;
}

int syn_refine_landmarks(syn_handle *h, const float *param, const float *pool, int B, int transform, const float *roi, float *lmk_coarse,
                         float *lmk_refined, float *global_feat, void *stream) {
    if (!h || !param || !pool || !lmk_refined) return fail(SYN_ERR_INVALID, "syn_refine_landmarks: NULL argument");
    if (B <= 0) return fail(SYN_ERR_INVALID, "syn_refine_landmarks: B=%d", B);
    int rc = synergy_ready(h, "syn_refine_landmarks");
    if (rc != SYN_OK) return rc;
    if (!h->d_basis) return fail(SYN_ERR_NOT_LOADED, "syn_refine_landmarks: 3DMM basis not loaded");
    if (h->n_lmk != syn::kSynPts) return fail(SYN_ERR_INVALID, "syn_refine_landmarks: the landmark basis has %d points, the MLPs take %d", h->n_lmk, syn::kSynPts);
    if (lmk_coarse && overlap(lmk_coarse, lmk_refined, kSwsLc * B)) return fail(SYN_ERR_INVALID, "syn_refine_landmarks: lmk_coarse overlaps lmk_refined");
    DeviceGuard g(h->device);
    rc = ensure_sws(h, kSwsPerFace * B * sizeof(float));
    if (rc != SYN_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    float *Lc = h->sws;
    // crop-space Lc with syn_landmarks_pose's own kernel (no pose: angles == null); with a ROI the caller's coarse copy is that kernel's
    // ROI output, so that it equals syn_landmarks_pose(roi) bit for bit
    syn::launch_lmk_pose(param, basis_mean(h), basis_std(h), basis_lmk(h), h->n_lmk, h->nlp, nullptr, transform, Lc, nullptr, nullptr, B, s);
    if (lmk_coarse) {
        if (roi) syn::launch_lmk_pose(param, basis_mean(h), basis_std(h), basis_lmk(h), h->n_lmk, h->nlp, roi, transform, lmk_coarse, nullptr, nullptr, B, s);
        else HIP_TRY(hipMemcpyAsync(lmk_coarse, Lc, kSwsLc * B * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    return run_refine(h, Lc, pool, param, B, roi, lmk_refined, global_feat, s);
}

int syn_refine_points(syn_handle *h, const float *lmk, const float *pool, const float *param, int B, float *lmk_refined, float *global_feat,
                      void *stream) {
    if (!h || !lmk || !pool || !param || !lmk_refined) return fail(SYN_ERR_INVALID, "syn_refine_points: NULL argument");
    if (B <= 0) return fail(SYN_ERR_INVALID, "syn_refine_points: B=%d", B);
    int rc = synergy_ready(h, "syn_refine_points");
    if (rc != SYN_OK) return rc;
    if (overlap(lmk, lmk_refined, kSwsLc * B)) return fail(SYN_ERR_INVALID, "syn_refine_points: lmk_refined overlaps lmk");
    DeviceGuard g(h->device);
    rc = ensure_sws(h, kSwsPerFace * B * sizeof(float));
    if (rc != SYN_OK) return rc;
    return run_refine(h, lmk, pool, param, B, nullptr, lmk_refined, global_feat, (hipStream_t)stream);
}

int syn_landmarks_to_param(syn_handle *h, const float *lmk, int B, float *param, void *stream) {
    if (!h || !lmk || !param) return fail(SYN_ERR_INVALID, "syn_landmarks_to_param: NULL argument");
    if (B <= 0) return fail(SYN_ERR_INVALID, "syn_landmarks_to_param: B=%d", B);
    int rc = synergy_ready(h, "syn_landmarks_to_param");
    if (rc != SYN_OK) return rc;
    DeviceGuard g(h->device);
    rc = ensure_sws(h, kSwsPerFace * B * sizeof(float));
    if (rc != SYN_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    float *gf = h->sws + (kSwsPerFace - kSwsGf) * B;
    const SynOffsets &o = h->syn_off;
    syn::launch_syn_trunk(trunk_weights(h, 1), lmk, B, nullptr, gf, syn::kSynGlobal, nullptr, s);
    syn::launch_syn_face_gemm(gf, syn::kSynGlobal, h->d_syn + o.Wrev, syn::kSynGlobal, h->d_syn + o.scale_rev, h->d_syn + o.shift_rev, param,
                              SYN_PARAM_DIM, SYN_PARAM_DIM, B, s);
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

// ---------------------------------------------------------------------------------------------
// Losses of the training graph's forward (model_building.py:141-157) and the benchmark loader's CenterCrop (kernels: loss_kernels.hip)
// ---------------------------------------------------------------------------------------------
int syn_wing_loss(syn_handle *h, const float *pred, const float *target, int B, int n_points, float omega, float epsilon, float *loss,
                  void *stream) {
    if (!h || !pred || !target || !loss) return fail(SYN_ERR_INVALID, "syn_wing_loss: NULL argument");
    if (B <= 0) return fail(SYN_ERR_INVALID, "syn_wing_loss: B=%d", B);
    if (n_points < 1) return fail(SYN_ERR_INVALID, "syn_wing_loss: n_points=%d", n_points);
    if (!(omega > 0.f) || !(epsilon > 0.f)) return fail(SYN_ERR_INVALID, "syn_wing_loss: omega=%g epsilon=%g", (double)omega, (double)epsilon);
    DeviceGuard g(h->device);
    const size_t N = (size_t)B * 3 * (size_t)n_points;
    int rc = ensure_sws(h, (size_t)syn::wing_chunks(N) * 2 * sizeof(double));
    if (rc != SYN_OK) return rc;
    syn::launch_wing_loss(pred, target, N, omega, epsilon, (double *)h->sws, loss_counter(h), loss, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

int syn_param_loss(syn_handle *h, const float *input, const float *target, int B, int mode, float *loss, void *stream) {
    if (!h || !input || !target || !loss) return fail(SYN_ERR_INVALID, "syn_param_loss: NULL argument");
    if (B <= 0) return fail(SYN_ERR_INVALID, "syn_param_loss: B=%d", B);
    if (mode != 0 && mode != 1) return fail(SYN_ERR_INVALID, "syn_param_loss: mode=%d (0 normal, 1 only_3dmm)", mode);
    DeviceGuard g(h->device);
    syn::launch_param_loss(input, target, B, mode, loss, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

int syn_synergy_losses(syn_handle *h, const float *param, const float *target, const float *pool, int B, float *scalars, float *per_face,
                       double *meter, void *stream) {
    if (!h || !param || !target || !pool || !scalars || !per_face) return fail(SYN_ERR_INVALID, "syn_synergy_losses: NULL argument");
    if (B <= 0) return fail(SYN_ERR_INVALID, "syn_synergy_losses: B=%d", B);
    int rc = synergy_ready(h, "syn_synergy_losses");
    if (rc != SYN_OK) return rc;
    if (!h->d_basis) return fail(SYN_ERR_NOT_LOADED, "syn_synergy_losses: 3DMM basis not loaded");
    if (h->n_lmk != syn::kSynPts) return fail(SYN_ERR_INVALID, "syn_synergy_losses: the landmark basis has %d points, the MLPs take %d", h->n_lmk, syn::kSynPts);
    DeviceGuard g(h->device);
    // behind the refinement's scratch: Lgt [B,3,68] | Lr [B,3,68] | param_rev [B,64] | chunk sums [groups][8] doubles
    const size_t groups = syn::loss_groups(B);
    rc = ensure_sws(h, (kSwsPerFace + 2 * kSwsLc + 64) * B * sizeof(float) + groups * 8 * sizeof(double));
    if (rc != SYN_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    float *Lc = h->sws, *Lgt = h->sws + kSwsPerFace * B, *Lr = Lgt + kSwsLc * B, *prev = Lr + kSwsLc * B;
    double *partial = (double *)(prev + (size_t)64 * B);
    syn::launch_lmk_pose(param, basis_mean(h), basis_std(h), basis_lmk(h), h->n_lmk, h->nlp, nullptr, 1, Lc, nullptr, nullptr, B, s);
    syn::launch_lmk_pose(target, basis_mean(h), basis_std(h), basis_lmk(h), h->n_lmk, h->nlp, nullptr, 1, Lgt, nullptr, nullptr, B, s);
    rc = run_refine(h, Lc, pool, param, B, nullptr, Lr, nullptr, s);
    if (rc != SYN_OK) return rc;
    float *gf = h->sws + (kSwsPerFace - kSwsGf) * B;
    const SynOffsets &o = h->syn_off;
    syn::launch_syn_trunk(trunk_weights(h, 1), Lr, B, nullptr, gf, syn::kSynGlobal, nullptr, s);
    syn::launch_syn_face_gemm(gf, syn::kSynGlobal, h->d_syn + o.Wrev, syn::kSynGlobal, h->d_syn + o.scale_rev, h->d_syn + o.shift_rev, prev,
                              SYN_PARAM_DIM, SYN_PARAM_DIM, B, s);
    syn::launch_synergy_losses(param, target, Lc, Lgt, Lr, prev, B, partial, loss_counter(h), scalars, per_face, meter, s);
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

// Backward of the two loss modules (kernels: loss_backward_kernels.hip)
int syn_wing_loss_backward(syn_handle *h, const float *pred, const float *target, int B, int n_points, float omega, float epsilon, const float *g,
                           float *d_pred, void *stream) {
    if (!h || !pred || !target || !d_pred) return fail(SYN_ERR_INVALID, "syn_wing_loss_backward: NULL argument");
    if (B <= 0) return fail(SYN_ERR_INVALID, "syn_wing_loss_backward: B=%d", B);
    if (n_points < 1) return fail(SYN_ERR_INVALID, "syn_wing_loss_backward: n_points=%d", n_points);
    if (!(omega > 0.f) || !(epsilon > 0.f))
        return fail(SYN_ERR_INVALID, "syn_wing_loss_backward: omega=%g epsilon=%g", (double)omega, (double)epsilon);
    DeviceGuard guard(h->device);
    const size_t N = (size_t)B * 3 * (size_t)n_points;
    int rc = ensure_sws(h, ((size_t)syn::wing_chunks(N) + 1) * sizeof(unsigned long long));      // chunk counts | n
    if (rc != SYN_OK) return rc;
    syn::launch_wing_loss_backward(pred, target, N, omega, epsilon, g, (unsigned long long *)h->sws, loss_counter(h), d_pred, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

int syn_param_loss_backward(syn_handle *h, const float *input, const float *target, int B, int mode, const float *g, float *d_input,
                            float *d_target, void *stream) {
    if (!h || !input || !target) return fail(SYN_ERR_INVALID, "syn_param_loss_backward: NULL argument");
    if (!d_input && !d_target) return fail(SYN_ERR_INVALID, "syn_param_loss_backward: NULL argument (d_input and d_target: at least one output)");
    if (B <= 0) return fail(SYN_ERR_INVALID, "syn_param_loss_backward: B=%d", B);
    if (mode != 0 && mode != 1) return fail(SYN_ERR_INVALID, "syn_param_loss_backward: mode=%d (0 normal, 1 only_3dmm)", mode);
    DeviceGuard guard(h->device);
    syn::launch_param_loss_backward(input, target, B, mode, g, d_input, d_target, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

// The loss head's backward: the forward launches of syn_synergy_losses (without MLP_rev's and the loss launch), the two WingLoss counts,
// then per pass of at most kHeadGroupsMax faces the four phases of head_backward_kernel with the per-face GEMMs across faces between
// them (loss_backward_kernels.hip).  Scratch: the forward's | 2 x (chunks + 1) counts | per-face vectors | the pass's images.
// With d_flat (syn_synergy_losses_backward_weights) the phases also leave the unscaled gradients, every pass is followed
// by the weight products across its faces (loss_wgrad_kernels.hip) and the call ends with the launch that writes d_flat; behind the
// scratch above: the images of unscaled gradients | two more per-face vectors | the accumulators | d_param / d_pool where not given.
static int losses_backward_impl(const char *who, syn_handle *h, const float *param, const float *target, const float *pool, int B,
                                const float *g_scalars, const float *g_per_face, float *d_param, float *d_pool, float *d_flat, void *stream) {
    const bool wgt = d_flat != nullptr;
    int rc = synergy_ready(h, who);
    if (rc != SYN_OK) return rc;
    if (!h->d_basis) return fail(SYN_ERR_NOT_LOADED, "%s: 3DMM basis not loaded", who);
    if (h->n_lmk != syn::kSynPts) return fail(SYN_ERR_INVALID, "%s: the landmark basis has %d points, the MLPs take %d", who, h->n_lmk, syn::kSynPts);
    DeviceGuard guard(h->device);
    const size_t N = (size_t)B * kSwsLc, chunks = syn::wing_chunks(N);
    int pass = syn::kHeadGroupsMax;
    if (wgt) {
        const long long k = syn::test_knob("wgrad_pass", syn::kHeadWgPass);
        pass = k < 1 ? 1 : k > syn::kHeadGroupsMax ? syn::kHeadGroupsMax : (int)k;
    }
    const int groups = B < pass ? B : pass;
    int chunk = 1;
    if (wgt) {
        const long long k = syn::test_knob("wgrad_chunk", syn::kHeadWgChunk);
        chunk = k < 1 ? 1 : k > groups ? groups : (int)k;
    }
    const size_t fwd_floats = ((kSwsPerFace + 2 * kSwsLc + 64) * B + 3) / 4 * 4, count_words = (2 * (chunks + 1) + 1) / 2 * 2;
    const size_t face_floats = (size_t)syn::kHeadFaceFloats * B;
    const size_t wg_floats = wgt ? (size_t)groups * syn::kHeadWg + (size_t)(64 + 512) * B + syn::head_wgrad_acc_floats() + syn::head_wgrad_part_floats(groups, chunk) +
                                       (d_param ? 0 : (size_t)64 * B) + (d_pool ? 0 : (size_t)syn::kPool * B)
                                 : 0;
    rc = ensure_sws(h, (fwd_floats + face_floats + (size_t)groups * syn::kHeadWs + wg_floats) * sizeof(float) + count_words * sizeof(unsigned long long));
    if (rc != SYN_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    float *Lc = h->sws, *Lgt = h->sws + kSwsPerFace * B, *Lr = Lgt + kSwsLc * B;
    unsigned long long *count = (unsigned long long *)(h->sws + fwd_floats);
    syn::launch_lmk_pose(param, basis_mean(h), basis_std(h), basis_lmk(h), h->n_lmk, h->nlp, nullptr, 1, Lc, nullptr, nullptr, B, s);
    syn::launch_lmk_pose(target, basis_mean(h), basis_std(h), basis_lmk(h), h->n_lmk, h->nlp, nullptr, 1, Lgt, nullptr, nullptr, B, s);
    rc = run_refine(h, Lc, pool, param, B, nullptr, Lr, nullptr, s);
    if (rc != SYN_OK) return rc;
    syn::launch_wing_count(Lc, Lgt, N, 10.f, count, loss_counter(h), s);
    syn::launch_wing_count(Lr, Lgt, N, 10.f, count + chunks + 1, loss_counter(h), s);
    const SynOffsets &o = h->syn_off;
    const float *d = h->d_syn;
    syn::HeadBwdArgs a;
    a.tf = trunk_weights(h, 0);
    a.tr = trunk_weights(h, 1);
    a.hw = {d + o.W6p, d + o.scale6, d + o.shift6, d + o.W7, d + o.scale7, d + o.shift7, d + o.W8, d + o.scale8, d + o.shift8,
            d + o.W9, d + o.scale9, d + o.shift9};
    a.W6f = d + o.W6f; a.Wrev = d + o.Wrev; a.sc_rev = d + o.scale_rev; a.sh_rev = d + o.shift_rev;
    a.mean = basis_mean(h); a.stdv = basis_std(h); a.basis = basis_lmk(h);
    a.param = param; a.target = target;
    a.Lc = Lc; a.Lgt = Lgt; a.Lr = Lr; a.pf = h->sws + kSwsLc * B; a.G6 = h->sws + (kSwsLc + kSwsPf + kSwsX6) * B;
    a.n0 = count + chunks; a.n1 = count + 2 * chunks + 1;
    a.g_scalars = g_scalars; a.g_per_face = g_per_face;
    float *pf = (float *)(count + count_words);              // per-face vectors between the launches, then the workgroups' images
    a.GFRg = pf; a.S2g = a.GFRg + (size_t)syn::kSynGlobal * B; a.GS2g = a.S2g + (size_t)64 * B; a.DPARg = a.GS2g + (size_t)64 * B;
    a.DGFRg = a.DPARg + (size_t)64 * B; a.DG6g = a.DGFRg + (size_t)syn::kSynGlobal * B; a.DX6g = a.DG6g + (size_t)512 * B;
    a.ws = pf + face_floats;
    a.d_param = d_param; a.d_pool = d_pool; a.B = B;
    syn::HeadWgAcc acc = {};
    if (wgt) {
        a.wg = a.ws + (size_t)groups * syn::kHeadWs;
        a.GS2Ug = a.wg + (size_t)groups * syn::kHeadWg;
        a.DG6Ug = a.GS2Ug + (size_t)64 * B;
        float *p = a.DG6Ug + (size_t)512 * B;
        syn::head_wgrad_acc_carve(p, acc);
        p += syn::head_wgrad_acc_floats();
        acc.part = p;
        acc.chunk = chunk;
        p += syn::head_wgrad_part_floats(groups, chunk);
        if (!d_param) { a.d_param = p; p += (size_t)64 * B; }
        if (!d_pool) a.d_pool = p;
    }
    const float *X6 = h->sws + (kSwsLc + kSwsPf) * B;
    for (int b0 = 0; b0 < B; b0 += groups) {                 // a pass of at most kHeadGroupsMax faces: the images are reused by the next one
        const int nb = B - b0 < groups ? B - b0 : groups;
        syn::launch_head_backward_phase(0, a, b0, nb, s);
        syn::launch_syn_face_gemm(a.GFRg + (size_t)syn::kSynGlobal * b0, syn::kSynGlobal, a.Wrev, syn::kSynGlobal, a.sc_rev, a.sh_rev,
                                  a.S2g + (size_t)64 * b0, 64, SYN_PARAM_DIM, nb, s);
        syn::launch_head_backward_phase(1, a, b0, nb, s);
        syn::launch_face_tgemm(a.GS2g + (size_t)64 * b0, 64, a.Wrev, syn::kSynGlobal, 64, a.DGFRg + (size_t)syn::kSynGlobal * b0, syn::kSynGlobal,
                               syn::kSynGlobal, nb, s);
        syn::launch_head_backward_phase(2, a, b0, nb, s);
        syn::launch_face_tgemm(a.DG6g + (size_t)512 * b0, 512, a.W6f, syn::kSynFaceKpad, 512, a.DX6g + (size_t)syn::kSynFaceKpad * b0,
                               syn::kSynFaceKpad, syn::kSynFaceKpad, nb, s);
        syn::launch_head_backward_phase(3, a, b0, nb, s);
        if (wgt) syn::launch_head_wgrad_pass(a, acc, X6, b0, nb, b0 == 0, s);
    }
    if (wgt) syn::launch_head_wgrad_final(acc, h->d_syn_flat, d_flat, s);
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

int syn_synergy_losses_backward(syn_handle *h, const float *param, const float *target, const float *pool, int B, const float *g_scalars,
                                const float *g_per_face, float *d_param, float *d_pool, void *stream) {
    if (!h || !param || !target || !pool || !d_param || !d_pool) return fail(SYN_ERR_INVALID, "syn_synergy_losses_backward: NULL argument");
    if ((g_scalars == nullptr) != (g_per_face == nullptr))
        return fail(SYN_ERR_INVALID, "syn_synergy_losses_backward: g_scalars and g_per_face are NULL together (the loss_total gradient) or not at all");
    if (B <= 0) return fail(SYN_ERR_INVALID, "syn_synergy_losses_backward: B=%d", B);
    return losses_backward_impl("syn_synergy_losses_backward", h, param, target, pool, B, g_scalars, g_per_face, d_param, d_pool, nullptr, stream);
}

// Weight gradients of MLP_for / MLP_rev in the flat layout; d_param / d_pool are optional here
int syn_synergy_losses_backward_weights(syn_handle *h, const float *param, const float *target, const float *pool, int B, const float *g_scalars,
                                        const float *g_per_face, float *d_param, float *d_pool, float *d_flat, void *stream) {
    if (!h || !param || !target || !pool || !d_flat) return fail(SYN_ERR_INVALID, "syn_synergy_losses_backward_weights: NULL argument");
    if ((g_scalars == nullptr) != (g_per_face == nullptr))
        return fail(SYN_ERR_INVALID,
                    "syn_synergy_losses_backward_weights: g_scalars and g_per_face are NULL together (the loss_total gradient) or not at all");
    if (B <= 0) return fail(SYN_ERR_INVALID, "syn_synergy_losses_backward_weights: B=%d", B);
    return losses_backward_impl("syn_synergy_losses_backward_weights", h, param, target, pool, B, g_scalars, g_per_face, d_param, d_pool, d_flat,
                                stream);
}

// Replaces the handle's MLP weights from a flat state on the device: a copy into the handle's flat image, then one launch that folds
// (fp64, one rounding, as fold_mlp) and repacks into the buffers and at the offsets syn_load_synergy set up.  Stream-ordered, no host
// synchronisation.
static syn::SynFoldTable synergy_fold_table(const syn_handle *h);
int syn_update_synergy_device(syn_handle *h, const float *flat_dev, size_t n, void *stream) {
    if (!h || !flat_dev) return fail(SYN_ERR_INVALID, "syn_update_synergy_device: NULL argument");
    if (n != synergy_flat_count()) return fail(SYN_ERR_INVALID, "syn_update_synergy_device: %zu floats, expected %zu", n, synergy_flat_count());
    if (!h->d_syn || !h->d_syn_flat) return fail(SYN_ERR_NOT_LOADED, "syn_update_synergy_device: synergy weights not loaded (syn_load_synergy sets up the buffers)");
    DeviceGuard guard(h->device);
    hipStream_t s = (hipStream_t)stream;
    if (flat_dev != h->d_syn_flat) HIP_TRY(hipMemcpyAsync(h->d_syn_flat, flat_dev, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    syn::launch_syn_fold_device(h->d_syn_flat, h->d_syn, synergy_fold_table(h), s);
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

// where the fold launch puts each layer of the flat state: the buffers and offsets syn_load_synergy set up
static syn::SynFoldTable synergy_fold_table(const syn_handle *h) {
    const SynOffsets &o = h->syn_off;
    syn::SynFoldTable t;
    auto set = [&t](int i, size_t W, int ld, size_t sc, size_t sh) { t.L[i] = {W, 0, sc, sh, ld, 0, syn::syn_flat_layer(i).K}; };
    for (int which = 0; which < 2; ++which)
        for (int i = 0; i < 5; ++i) set(which * 9 + i, o.tW[which][i], i == 0 ? 4 : syn::syn_flat_layer(i).K, o.tscale[which][i], o.tshift[which][i]);
    t.L[5] = {o.W6p, o.W6f, o.scale6, o.shift6, 64, syn::kSynFaceKpad, 64};
    set(6, o.W7, 512, o.scale7, o.shift7);
    set(7, o.W8, 256, o.scale8, o.shift8);
    set(8, o.W9, 128, o.scale9, o.shift9);
    int row = 0;
    for (int i = 14; i < 17; ++i) {
        set(i, o.Wrev + (size_t)row * 1024, 1024, o.scale_rev + row, o.shift_rev + row);
        row += syn::syn_flat_layer(i).N;
    }
    return t;
}

size_t syn_synergy_bn_channels(void) { return (size_t)syn::kSynBnChannels; }

// The inverse of syn_update_synergy_device: the handle's flat state (with the running statistics syn_synergy_losses_train moved) copied
// device to device, stream-ordered.
int syn_export_synergy_flat(syn_handle *h, float *flat_dev, size_t n, void *stream) {
    if (!h || !flat_dev) return fail(SYN_ERR_INVALID, "syn_export_synergy_flat: NULL argument");
    if (n != synergy_flat_count()) return fail(SYN_ERR_INVALID, "syn_export_synergy_flat: %zu floats, expected %zu", n, synergy_flat_count());
    if (!h->d_syn || !h->d_syn_flat) return fail(SYN_ERR_NOT_LOADED, "syn_export_synergy_flat: synergy weights not loaded (syn_load_synergy)");
    DeviceGuard guard(h->device);
    HIP_TRY(hipMemcpyAsync(flat_dev, h->d_syn_flat, n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return SYN_OK;
}

static bool bytes_overlap(const void *a, size_t na, const void *b, size_t nb) {
    const char *x = (const char *)a, *y = (const char *)b;
    return a && b && x < y + nb && y < x + na;
}

// syn_synergy_losses with every BatchNorm of MLP_for / MLP_rev normalising by the statistics of the batch (the reference in train();
// kernels: loss_train_kernels.hip).  Scratch: Lc | Lgt | Lr | S2 [B,64] | the layer images (train_scratch_floats) | the
// blocks' partial sums | the loss launch's chunk sums.
int syn_synergy_losses_train(syn_handle *h, const float *param, const float *target, const float *pool, int B, float *scalars, float *per_face,
                             double *meter, float *batch_stats, float momentum, void *stream) {
    if (!h || !param || !target || !pool || !scalars || !per_face) return fail(SYN_ERR_INVALID, "syn_synergy_losses_train: NULL argument");
    if (B < 2)
        return fail(SYN_ERR_INVALID, "syn_synergy_losses_train: B=%d: Expected more than 1 value per channel when training, got input size [%d, 12, 1]",
                    B, B);
    if (B > syn::kTrainMaxFaces) return fail(SYN_ERR_INVALID, "syn_synergy_losses_train: B=%d, at most %d faces per call", B, syn::kTrainMaxFaces);
    if (!(momentum <= 1.f)) return fail(SYN_ERR_INVALID, "syn_synergy_losses_train: momentum=%g, expected 0..1 (or negative: running statistics untouched)", (double)momentum);
    int rc = synergy_ready(h, "syn_synergy_losses_train");
    if (rc != SYN_OK) return rc;
    if (!h->d_basis) return fail(SYN_ERR_NOT_LOADED, "syn_synergy_losses_train: 3DMM basis not loaded");
    if (h->n_lmk != syn::kSynPts) return fail(SYN_ERR_INVALID, "syn_synergy_losses_train: the landmark basis has %d points, the MLPs take %d", h->n_lmk, syn::kSynPts);
    const size_t n_sc = 2 * sizeof(float), n_pf = (size_t)3 * B * sizeof(float), n_bs = 2 * (size_t)syn::kSynBnChannels * sizeof(float), n_mt = 8 * sizeof(double);
    if (bytes_overlap(scalars, n_sc, per_face, n_pf) || bytes_overlap(scalars, n_sc, batch_stats, n_bs) || bytes_overlap(per_face, n_pf, batch_stats, n_bs) ||
        bytes_overlap(meter, n_mt, scalars, n_sc) || bytes_overlap(meter, n_mt, per_face, n_pf) || bytes_overlap(meter, n_mt, batch_stats, n_bs))
        return fail(SYN_ERR_INVALID, "syn_synergy_losses_train: the outputs overlap");
    DeviceGuard g(h->device);
    const long long knob = syn::test_knob("train_rows", syn::kTrainRows);
    const int rows = knob < 16 ? 16 : knob > (1 << 20) ? (1 << 20) : (int)knob;
    const size_t groups = syn::loss_groups(B);
    const size_t head_floats = (3 * kSwsLc + 64) * B, train_floats = syn::train_scratch_floats(B), part_doubles = syn::train_part_doubles(B, rows);
    rc = ensure_sws(h, (head_floats + train_floats) * sizeof(float) + (part_doubles + groups * 8) * sizeof(double));
    if (rc != SYN_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    float *Lc = h->sws, *Lgt = Lc + kSwsLc * B, *Lr = Lgt + kSwsLc * B, *prev = Lr + kSwsLc * B;
    syn::SynTrainArgs a = {};
    a.scratch = prev + (size_t)64 * B;
    a.part = (double *)(a.scratch + train_floats);
    double *partial = a.part + part_doubles;
    const SynOffsets &o = h->syn_off;
    const float *d = h->d_syn;
    for (int which = 0; which < 2; ++which)
        for (int i = 0; i < 5; ++i) a.Wt[which][i] = d + o.tW[which][i];
    a.W6p = d + o.W6p; a.W6f = d + o.W6f; a.W7 = d + o.W7; a.W8 = d + o.W8; a.W9 = d + o.W9; a.Wrev = d + o.Wrev;
    a.flat = h->d_syn_flat;
    a.Lc = Lc; a.pool = pool; a.param = param; a.Lr = Lr; a.S2 = prev;
    a.batch_stats = batch_stats; a.momentum = momentum; a.B = B; a.rows = rows;
    syn::launch_lmk_pose(param, basis_mean(h), basis_std(h), basis_lmk(h), h->n_lmk, h->nlp, nullptr, 1, Lc, nullptr, nullptr, B, s);
    syn::launch_lmk_pose(target, basis_mean(h), basis_std(h), basis_lmk(h), h->n_lmk, h->nlp, nullptr, 1, Lgt, nullptr, nullptr, B, s);
    syn::launch_synergy_train_head(a, s);
    syn::launch_synergy_losses(param, target, Lc, Lgt, Lr, prev, B, partial, loss_counter(h), scalars, per_face, meter, s);
    if (momentum >= 0.f) syn::launch_syn_fold_device(h->d_syn_flat, h->d_syn, synergy_fold_table(h), s);      // every eval() entry sees the moved statistics
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

int syn_center_crop_u8(syn_handle *h, const uint8_t *in, int B, int H, int W, int C, int margin, uint8_t *out, void *stream) {
    if (!h || !in || !out) return fail(SYN_ERR_INVALID, "syn_center_crop_u8: NULL argument");
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0) return fail(SYN_ERR_INVALID, "syn_center_crop_u8: B=%d H=%d W=%d C=%d", B, H, W, C);
    if (margin < 0) return fail(SYN_ERR_INVALID, "syn_center_crop_u8: margin=%d", margin);
    DeviceGuard g(h->device);
    syn::launch_center_crop_u8(in, out, B, H, W, C, margin, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

int syn_train_transform_u8(syn_handle *h, const uint8_t *src, int N, int H, int W, const syn_train_record *records, int B, int margin, float mean,
                           float std, float *out_f32, uint8_t *out_u8, void *stream) {
    if (!h || !src || !records) return fail(SYN_ERR_INVALID, "syn_train_transform_u8: NULL argument");
    if (!out_f32 && !out_u8) return fail(SYN_ERR_INVALID, "syn_train_transform_u8: both outputs are NULL");
    if (N <= 0 || H <= 0 || W <= 0 || B <= 0) return fail(SYN_ERR_INVALID, "syn_train_transform_u8: N=%d H=%d W=%d B=%d", N, H, W, B);
    if (margin < 0) return fail(SYN_ERR_INVALID, "syn_train_transform_u8: margin=%d", margin);
    if (!std::isfinite(std) || std == 0.f || !std::isfinite(mean)) return fail(SYN_ERR_INVALID, "syn_train_transform_u8: mean=%g std=%g", mean, std);
    const unsigned long long face = 3ull * (unsigned long long)H * (unsigned long long)W;
    if (face > SYN_TRAIN_TRANSFORM_MAX_FACE_BYTES)
        return fail(SYN_ERR_INVALID, "syn_train_transform_u8: a face of %llu bytes (H=%d W=%d) does not fit one workgroup's LDS, at most %d", face, H, W,
                    SYN_TRAIN_TRANSFORM_MAX_FACE_BYTES);
    const size_t n_src = (size_t)N * face, n_u8 = (size_t)B * face, n_f32 = n_u8 * sizeof(float);
    if (bytes_overlap(out_f32, n_f32, src, n_src) || bytes_overlap(out_u8, n_u8, src, n_src) || bytes_overlap(out_f32, n_f32, out_u8, n_u8))
        return fail(SYN_ERR_INVALID, "syn_train_transform_u8: an output overlaps the source set or the other output");
    DeviceGuard g(h->device);
    HIP_TRY(syn::launch_train_transform(src, N, H, W, records, B, margin, mean, std, out_f32, out_u8, (hipStream_t)stream));
    HIP_TRY(hipGetLastError());
    return SYN_OK;
}

}  // extern "C"
