// Register-resident fused inverted-residual block for the 4x4 MobileNetV2 blocks (features.15-17: 160 -> 960 -> 160 | 320).
// Reference: backbone_nets/mobilenetv2_backbone.py:45-74 (InvertedResidual.forward), :33-42 (ConvBNReLU).
//
// Same idea as fused_block_lb.hip (hidden activations never leave registers, fp16 x2 operands, three partial products per MAC),
// re-cut for a block whose weights (1.2 / 1.8 MB as fragments) dwarf its activations (10 KB per face):
//
//   * one WAVE = one face = one 16-column block of v_mfma_f32_16x16x32_f16 (lane column n = 4y + x): the vertical neighbours of a
//     pixel are row_shr:4 / row_shl:4 inside the 16-lane DPP row (zero fill = the image border), the horizontal ones
//     row_shr:1 / row_shl:1 with the filter column zeroed where the shift crosses x = 0 | 3;
//   * the block input of the face lives in REGISTERS as pre-split B fragments (5 k32 steps x 2 pieces = 40 registers), the
//     accumulators too: the waves walk the 30 hidden groups with no partial sums to exchange;
//   * the WEIGHTS go through LDS: the eight waves of a workgroup (four faces) walk the groups in lockstep and share one fetch of each group's
//     fragments + constants -- one contiguous 48 | 64 KB run of the packed blob, an eighth per wave, loaded STRAIGHT into the other half of
//     a double buffer (buffer loads with the lds modifier: 1 KB per wave-instruction, no staging registers, no ds_write), the expand part
//     two groups ahead, the project part one, issued between the matrix instructions of the expand chain and published by counted
//     s_waitcnt vmcnt in front of the two barriers of a group; the group's expand operands are requested from LDS while the previous
//     group's project runs, its project fragments inside its own expand chain: no LDS phase stands between the last matrix instruction
//     of a group and the first of the next (lb4_stage).
//     (Each wave fetching its own fragments would pull 1.2 MB through L2 per face.)
//   * TWO waves per face (B = 1024 offers four faces per CU, and a lone wave per SIMD issues vector instructions at half the
//     rate): wave (face, t) owns hidden tile t through expand and depthwise and half of the output tiles in the project; the
//     two halves of the project operand cross through LDS (16 bytes per lane, one extra barrier per group).
// Scales as in fused_block_lb.hip: X16 = 16 x;  D = 16 Se (We x + shift);  E = med3(D, 0, 96 Se);  O16 = 16 dshift + sum (taps / Se) E;
// B = med3(O16, 0, 96);  acc = 16 Sp (Wp o);  y = acc / (16 Sp) + pshift (+ x).
#include "syn_internal.h"

#include <cstdio>
#include <cstdlib>
#include <type_traits>

namespace syn {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) void *lds_ptr_t;

namespace {
__device__ __forceinline__ void split2q(float x0, float x1, unsigned &a, unsigned &b) {
    // a = fp16 pair (toward zero); x - a in ONE v_fma_mix_f32 per value (fp16 source operand: no v_cvt_f32_f16)
    a = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(x0, x1));
    float r0, r1;
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(r0) : "v"(a), "v"(x0));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r1) : "v"(a), "v"(x1));
    b = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(r0, r1));
}
__device__ __forceinline__ void split2w(float x0, float x1, u32x4 (&pc)[2], int d) {
    unsigned a, b;
    split2q(x0, x1, a, b);
    pc[0][d] = a; pc[1][d] = b;
}
__device__ __forceinline__ f32x4 mfmaq(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
// (by value: __builtin_bit_cast of a vector ELEMENT reads element 0 whatever the index -- clang 19 / ROCm 7.2)
template <int CTRL>
__device__ __forceinline__ float dppq(float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), CTRL, 0xf, 0xf, true));
}
template <int CTRL>
__device__ __forceinline__ f32x2 dppq2(f32x2 v) {
    f32x2 r;
    r[0] = dppq<CTRL>(v[0]);
    r[1] = dppq<CTRL>(v[1]);
    return r;
}
constexpr int kShr1 = 0x111, kShl1 = 0x101, kShr4 = 0x114, kShl4 = 0x104;     // lane n <- n-1 | n+1 | n-4 | n+4 of its 16-lane row, else 0
}  // namespace

template <int CIN_, int HID_, int COUT_, bool RES_>
struct Lb4Cfg {
    static constexpr int CIN = CIN_, HID = HID_, COUT = COUT_;
    static constexpr bool RES = RES_;
    static constexpr int KE = CIN / 32, NG = HID / 32, MT = COUT / 16, MTW = MT / 2;         // MTW: output tiles per wave
    static constexpr int WE_DW = 2 * KE * 2 * 256, WP_DW = MT * 2 * 256, TB_DW = 2 * 256;   // a group's expand | project fragments | constants (12 x 32 floats + pad)
    static constexpr int NKB = ((WE_DW + WP_DW + TB_DW) / 256 + 7) / 8 * 8;               // 1 KB pieces per group, padded to one more round of the 8 waves (lb4_group_dwords)
    static constexpr int GRP_DW = NKB * 256;
    // the two parts a run is loaded in (lb4_dma), in 1 KB pieces: E = expand fragments + constants + two pieces of the padding (what a group
    // STARTS from), P = project fragments + the rest of the padding (what its expand chain asks for); per wave NE | NP pieces
    static constexpr int WEP = WE_DW / 256, WPP = WP_DW / 256, NE = (WEP + 4) / 8, NP = NKB / 8 - NE;
    static_assert((WEP + 4) % 8 == 0 && WEP + WPP + 4 <= NKB, "E = 24 pieces: every wave issues the same number, the vmcnt counts depend on it");
    static constexpr int XCH_DW = 4 * 2 * 64 * 4;                                         // depthwise outputs exchanged between the two waves of a face
    static constexpr int LDS_DW = 2 * GRP_DW + XCH_DW;
    static_assert(CIN % 32 == 0 && HID % 32 == 0 && COUT % 32 == 0, "k32 steps, groups, two halves of the output tiles");
    static_assert(!RES || CIN == COUT, "residual only on same-width blocks");
    static_assert(LDS_DW * 4 <= 160 * 1024, "LDS budget");
};

// Workgroup = 4 faces x 2 waves: wave (face, t) owns hidden tile t (16 of the group's 32 channels) through expand and depthwise,
// hands its half of the project operand to its partner through LDS, and accumulates half of the output tiles.  Two waves per SIMD
// issue vector instructions at 2.4 cycles each instead of a lone wave's 5 (the depthwise is the larger part of a group).
//
// One block = one STAGE; features.15-17 run as a chain of three stages in one launch (fused_chain_lb4_kernel): the block output goes
// to the next stage as pre-split fragments through the weight buffer half the last group has just left, the residual of the next block
// stays in the accumulator's registers, and the next stage's first weight group is fetched during the last group of this one --
// no kernel boundary (10-16 us each), no global round trip of the 4x4 activations.
struct Lb4NoNext { static constexpr int NKB = 0, NE = 0, NP = 0, GRP_DW = 0, NG = 0; };
struct Lb4StageArgs {
    const float *X;          // block input (global): a FIRST stage's input and residual
    const unsigned *Glb;     // [NG][NKB][64][4]: We | Wp | table per group
    const float *p_shift;
    float *Y;                // block output (global): written by the last stage only
    float *part = nullptr;   // hidden-sliced schedule: partial sums [slice][B][16][COUT] (raw accumulators)
    int g0 = 0, g1 = 0;      // hidden groups [g0, g1) of this workgroup's slice (g1 = 0: all); slice = blockIdx.y
};

// Piece I of this wave's share of part E | P of a group run (configuration C): global -> LDS with no register in between.  rs: the stage's
// blob; grp: byte offset of the group's run in it (uniform); half: where the run goes.  The LDS image is the run itself (lane-linear pieces).
// The padding pieces are loaded like the others so that EVERY wave has the same number of loads in flight.
// Nothing orders a ds_read behind such a load but the issuing wave's s_waitcnt vmcnt AND a barrier behind it (lb4_wait_vm, lb4_barrier).
template <class C, bool PPART, int I>
__device__ __forceinline__ void lb4_dma(__amdgpu_buffer_rsrc_t rs, unsigned grp, unsigned *half, unsigned lane16, int wave /* uniform */) {
    const int slot = wave + 8 * I;
    const int piece = PPART ? (slot < C::WPP ? C::WEP + slot : slot + C::WEP + 4) : (slot < C::WEP ? slot : slot + C::WPP);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr_t)(half + piece * 256), 16, lane16, grp + piece * 1024, 0, 0);
}
template <class C, bool PPART, int I0, int I1>
__device__ __forceinline__ void lb4_dma_range(__amdgpu_buffer_rsrc_t rs, unsigned grp, unsigned *half, unsigned lane16, int wave) {
    if constexpr (I0 < I1) {
        lb4_dma<C, PPART, I0>(rs, grp, half, lane16, wave);
        lb4_dma_range<C, PPART, I0 + 1, I1>(rs, grp, half, lane16, wave);
    }
}
template <class C>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t lb4_rsrc(const unsigned *Glb) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned *>(Glb), 0, C::NG * C::GRP_DW * 4, 0x00027000);
}
// all but the N youngest loads of this wave have landed (they return in order)
template <int N>
__device__ __forceinline__ void lb4_wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
// workgroup barrier that leaves the loads in flight (__syncthreads() would drain them): this wave's LDS reads and writes are done, nothing else
__device__ __forceinline__ void lb4_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// What a group's expand chain and depthwise start from, read from LDS one group AHEAD (during the previous group's project): the accumulator's
// start value, this wave's expand fragments, and rows 0-8 (filter taps) and 9 (BN shift) of the group's table for channels 16 t + 4 g .. + 3.
struct Lb4Pre {
    f32x4 D;
    u32x4 Ae[5][2];
    f32x4 wr[10];
};
constexpr int kLb4PreUnits = 10;     // eight registers each: units 0-4 = the k32 steps of Ae (0 with D in front), 5-9 = two table rows each
// unit u of group `half` (configuration C).  The LDS returns in order: the start value first, then the fragments in the order the chain consumes them.
template <class C>
__device__ __forceinline__ void lb4_pre_unit(Lb4Pre &pre, const unsigned *half, int u, int t, unsigned l4, unsigned g4) {
    if (u < 5) {
        const float *Tb = reinterpret_cast<const float *>(half + C::WE_DW + C::WP_DW);
        if (u == 0) pre.D = *(const f32x4 *)&Tb[10 * 32 + 16 * t + g4];
#pragma unroll
        for (int p = 1; p >= 0; --p) pre.Ae[u][p] = *(const u32x4 *)&half[((t * 5 + u) * 2 + p) * 256 + l4];
    } else {
        const float *Tb = reinterpret_cast<const float *>(half + C::WE_DW + C::WP_DW);
#pragma unroll
        for (int k = 2 * (u - 5); k < 2 * (u - 5) + 2; ++k) pre.wr[k] = *(const f32x4 *)&Tb[k * 32 + 16 * t + g4];
    }
}
template <class T> struct Lb4Tag { using type = T; };
template <int N> struct Lb4Int { static constexpr int value = N; };

// GRPL: dwords per half of the LDS weight double buffer (>= the group run of every stage of the kernel)
// PARTIAL (small batches): the workgroup (blockIdx.x = four faces, blockIdx.y = slice) walks only the hidden groups of its slice and
// stores its raw accumulators; lb4_reduce_kernel adds the slices in fixed order, rescales, adds BN shift and residual.  A batch of 128
// faces is then 32 x 6 workgroups of five groups each instead of 32 workgroups walking all thirty.
//
// The weight pipeline, per group G (two LDS halves; part E of a run = expand fragments + constants, part P = project fragments; `pre` = the
// next group's expand operands in registers):
//   top barrier          every wave is done with group G-1 and has its own reads of group G's operands back: the P part of G-1's half and the
//                        E part of G's OWN half (read for the last time under G-1's project) may be rewritten
//   expand chain         from `pre`; behind each k32 step one output tile's project fragments are requested from LDS and ONE piece is loaded
//                        global -> LDS: first P of G+1 (into G-1's half), then E of G+2 (into G's half); what is left, behind the chain
//   depthwise
//   vmcnt(NP + NE), exchange barrier   all but this group's loads have landed: it also publishes E of G+1 (issued a group ago)
//   PRE G+1              requested from LDS while G's project runs, into registers the project frees as it goes (PRE0 units up front,
//                        then one per output tile from tile LAG on, the rest behind the last)
//   vmcnt(NE)            P of G+1 has landed; the next top barrier publishes it.  E of G+2 stays in flight across it.
// The group a stage is entered with (G = gb) finds E and P of its own run in half 0 -- from the prologue (FIRST), or loaded by the last two
// groups of the stage in front -- and loads E of G+1 itself, in front of its chain: half 1 is the hand-over buffer between two stages, free
// only behind this group's top barrier.  At a stage's last two groups G+1 | G+2 are the NEXT stage's first groups (NG is even: its group 0
// goes to half 0).  Every wave issues the same number of loads per group and they return in order: the counts above hold whatever else is
// in flight.
template <class C, class CN, bool FIRST, int GRPL, bool PARTIAL, int PRE0, int LAG>
__device__ __forceinline__ void lb4_stage(unsigned *smem, const Lb4StageArgs &sa, const unsigned *GlbNext, int B, u32x4 (&Xr)[5][2], f32x4 (&vres)[5],
                                          Lb4Pre &pre) {
    constexpr int KE = C::KE, MTW = C::MTW, CIN = C::CIN, COUT = C::COUT;
    constexpr bool HANDOFF = !__is_same(CN, void);
    static_assert(KE == 5 && C::NG % 2 == 0, "160 input channels; the double buffer's parity carries over to the next stage");
    const float *__restrict__ X = sa.X, *__restrict__ p_shift = sa.p_shift;
    const unsigned *__restrict__ Glb = sa.Glb;
    float *__restrict__ Y = sa.Y;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fl = wave >> 1, t = wave & 1;
    const int f = blockIdx.x * 4 + fl;
    const bool real = f < B;
    const int fc = real ? f : B - 1;
    const int n = lane & 15, g = lane >> 4;
    const unsigned l4 = lane * 4, g4 = g * 4, l16 = lane * 16;
    unsigned *Xch = smem + 2 * GRPL;

    // every wave loads every eighth 1 KB piece of a part of a group's run straight into LDS (lb4_dma).  Measured with tools/ubench/lds_dma_stream.hip
    // (eight waves per CU, every CU, one shared 4.3 MB blob): 54 GB/s per CU with one piece in flight per wave, 110 with four, 115 with six or
    // eight -- four times what this kernel asks for (4.3 MB per CU in ~150 us = 29 GB/s).  (Round 2 read "25 GB/s per CU" off its own pace.)
    using CNX = typename std::conditional<HANDOFF, CN, Lb4NoNext>::type;
    const __amdgpu_buffer_rsrc_t rs = lb4_rsrc<C>(Glb), rsn = lb4_rsrc<CNX>(HANDOFF ? GlbNext : Glb);
    const int gsl = PARTIAL ? (sa.g1 - sa.g0) : C::NG;   // groups per slice (all slices the same)
    const int gb = PARTIAL ? (int)blockIdx.y * gsl : 0, ge = gb + gsl;
    if (FIRST) {
        lb4_dma_range<C, false, 0, C::NE>(rs, (unsigned)gb * (C::GRP_DW * 4), smem, l16, wave);
        lb4_dma_range<C, true, 0, C::NP>(rs, (unsigned)gb * (C::GRP_DW * 4), smem, l16, wave);
        // ---- block input of this face -> pre-split B fragments in registers (x 16; both waves of the face hold it) ----
        f32x4 xv[KE][2];
#pragma unroll
        for (int kc = 0; kc < KE; ++kc) {
            const float *src = X + ((size_t)fc * 16 + n) * CIN + 32 * kc + 8 * g;
            xv[kc][0] = *(const f32x4 *)src;
            xv[kc][1] = *(const f32x4 *)(src + 4);
        }
#pragma unroll
        for (int kc = 0; kc < KE; ++kc) {
            f32x4 a = xv[kc][0] * 16.0f, b = xv[kc][1] * 16.0f;
            if (!real) { a = (f32x4){0.f, 0.f, 0.f, 0.f}; b = a; }
            split2w(a[0], a[1], Xr[kc], 0);
            split2w(a[2], a[3], Xr[kc], 1);
            split2w(b[0], b[1], Xr[kc], 2);
            split2w(b[2], b[3], Xr[kc], 3);
        }
    }
    const float mL = (n & 3) != 0 ? 1.f : 0.f, mR = (n & 3) != 3 ? 1.f : 0.f;
    f32x4 acc[MTW];
#pragma unroll
    for (int i = 0; i < MTW; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float c6e = 0.f, inv_p = 0.f;
    if (FIRST) {
        lb4_wait_vm<0>();
        lb4_barrier();                                   // group gb is in half 0: its expand operands, which every later group finds requested by the group in front
#pragma unroll
        for (int u = 0; u < kLb4PreUnits; ++u) lb4_pre_unit<C>(pre, smem, u, t, l4, g4);
    }

    {   // ReLU6 ceiling of the scaled expand output, accumulator -> output: constants of the block, kept in group 0's table
        const float *t0 = reinterpret_cast<const float *>(Glb + C::WE_DW + C::WP_DW);
        c6e = t0[11 * 32]; inv_p = t0[11 * 32 + 1];
    }
    // One group.  Part P of the next group (configuration CP, blob rs1 at byte off1; void: there is no next group) and part E of the group after
    // next (C2, rs2, off2) are loaded, and the next group's expand operands requested in configuration CP: compile-time, so that every wave
    // issues a known number of loads.  The one uniform branch: the group a stage is entered with loads part E of its successor as well.
    auto group = [&](auto cp_, auto c2_, int G, __amdgpu_buffer_rsrc_t rs1, unsigned off1, __amdgpu_buffer_rsrc_t rs2, unsigned off2) __attribute__((always_inline)) {
        using CP = typename decltype(cp_)::type;
        using C2 = typename decltype(c2_)::type;
        constexpr bool HASNEXT = !__is_same(CP, void), HAS2 = !__is_same(C2, void);
        using CPX = typename std::conditional<HASNEXT, CP, Lb4NoNext>::type;
        using C2X = typename std::conditional<HAS2, C2, Lb4NoNext>::type;
        constexpr int NP1 = CPX::NP, NE2 = C2X::NE;
        static_assert(NP1 + NE2 <= 8, "dma_at");
        lb4_barrier();                                   // every wave is done with group G-1 (and has its own reads of group G's operands back)
        unsigned *Wg = smem + ((G - gb) & 1) * GRPL;       // the half of group G, whose E part is free from here on: then of group G+2
        const unsigned *Wp = Wg + C::WE_DW;
        unsigned *Wn = smem + ((G + 1 - gb) & 1) * GRPL;   // the half of group G-1, then of group G+1
        if constexpr (HASNEXT) {
            if (G == gb) lb4_dma_range<CPX, false, 0, CPX::NE>(rs1, off1, Wn, l16, wave);
        }
        // load j of this group: P of G+1 first (needed at the next top barrier), then E of G+2 (needed at the exchange barrier behind that)
        auto dma_j = [&](auto j_) __attribute__((always_inline)) {
            constexpr int J = decltype(j_)::value;
            if constexpr (J < NP1) lb4_dma<CPX, true, J>(rs1, off1, Wn, l16, wave);
            else if constexpr (J < NP1 + NE2) lb4_dma<C2X, false, J - NP1>(rs2, off2, Wg, l16, wave);
        };
        auto dma_at = [&](int j) __attribute__((always_inline)) {
            switch (j) {
                case 0: dma_j(Lb4Int<0>{}); break;
                case 1: dma_j(Lb4Int<1>{}); break;
                case 2: dma_j(Lb4Int<2>{}); break;
                case 3: dma_j(Lb4Int<3>{}); break;
                case 4: dma_j(Lb4Int<4>{}); break;
                case 5: dma_j(Lb4Int<5>{}); break;
                case 6: dma_j(Lb4Int<6>{}); break;
                case 7: dma_j(Lb4Int<7>{}); break;
                default: break;
            }
        };
        // Round 5: the eight waves read 22 KB each at this point, the LDS delivers 128 bytes per cycle, and the expand chain used to wait for ALL
        // of it: ~1400 cycles per group in which nothing else ran; then only the expand fragments stood in front of the chain.  Round 7: those
        // were requested during the previous group's project, so the chain starts here, and each k32 step of it is followed by the request of one
        // output tile's project fragments, into the registers that step's expand fragments have left: the LDS works under the chain instead of behind it.
        u32x4 Ap[MTW][2];
        f32x4 D = pre.D;
        constexpr int MTW0 = MTW > 5 ? MTW / 2 : MTW;    // (320 output channels: the second half of the project fragments after the exchange)
        static_assert(MTW0 == KE, "one output tile's project fragments per k32 step of the expand chain");
        // ---- expand 1x1 + BN shift: D = channels 32 G + 16 t + 4 g + i of pixel n (three partial products, smallest first) ----
#pragma unroll
        for (int kc = 0; kc < KE; ++kc) {
            D = mfmaq(pre.Ae[kc][1], Xr[kc][0], D);
            D = mfmaq(pre.Ae[kc][0], Xr[kc][1], D);
            D = mfmaq(pre.Ae[kc][0], Xr[kc][0], D);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int p = 0; p < 2; ++p) Ap[kc][p] = *(const u32x4 *)&Wp[((t * MTW + kc) * 2 + p) * 256 + l4];
            dma_at(kc);                                  // (memory instructions are issued in front of the matrix instructions that cover them, one at a time)
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int j = KE; j < NP1 + NE2; ++j) dma_at(j);
        __builtin_amdgcn_sched_barrier(0);
        // ---- ReLU6, depthwise 3x3 + BN shift + ReLU6 on the registers, split into this wave's half of the project operand ----
        u32x4 own;                                      // {piece 0 dwords hf 0, 1 | piece 1 dwords hf 0, 1}
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            // depthwise filter, its BN shift: two channels x two halves per lane group
            f32x2 w[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) w[k] = (f32x2){pre.wr[k][2 * hf], pre.wr[k][2 * hf + 1]};
            const f32x2 dsh = (f32x2){pre.wr[9][2 * hf], pre.wr[9][2 * hf + 1]};
            f32x2 E;
            // ReLU6 as clamp modifiers (fused_block_lb.hip): E = relu6 / 6 = clamp(D / (96 Se)); the last add of the output clamps too
            E[0] = __builtin_amdgcn_fmed3f(D[2 * hf] * c6e, 0.0f, 1.0f);
            E[1] = __builtin_amdgcn_fmed3f(D[2 * hf + 1] * c6e, 0.0f, 1.0f);
            // horizontal first (two lane shifts), then the three row sums shifted vertically (two more): 8 DPP moves per channel pair
            // instead of 16.  (Summation order differs from the other kernels': dx inside dy inside the vertical sum.)
            // the image border in x: the shifted VALUE is zeroed (two multiplies) instead of six filter entries -- the same products, bit for bit
            const f32x2 l = dppq2<kShr1>(E) * mL, rt = dppq2<kShl1>(E) * mR;
            f32x2 H[3];
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
                H[dy] = l * w[3 * dy];
                H[dy] += E * w[3 * dy + 1];
                H[dy] += rt * w[3 * dy + 2];
            }
            f32x2 O = dsh + dppq2<kShr4>(H[0]);          // kernel row 0 applies to the input row above: take it from lane n - 4
            O += H[1];
            {
                const f32x2 h2 = dppq2<kShl4>(H[2]);
                asm("v_pk_add_f32 %0, %1, %2 clamp" : "=v"(O) : "v"(O), "v"(h2));
            }
            unsigned a, b;
            split2q(O[0], O[1], a, b);
            own[hf] = a; own[2 + hf] = b;
        }
        // ---- the partner's half: K slots 0-3 of a lane group are tile 0's channels, 4-7 tile 1's ----
        *(u32x4 *)&Xch[((fl * 2 + t) * 64 + lane) * 4] = own;
        lb4_wait_vm<NP1 + NE2>();                        // this wave's pieces of part E of group G+1 (loaded a group ago, or in front of this chain) have landed
        lb4_barrier();                                   // the exchange; every wave's pieces of them are in LDS too
        const u32x4 oth = *(const u32x4 *)&Xch[((fl * 2 + (1 - t)) * 64 + lane) * 4];
#pragma unroll
        for (int i = MTW0; i < MTW; ++i)
#pragma unroll
            for (int p = 0; p < 2; ++p) Ap[i][p] = *(const u32x4 *)&Wp[((t * MTW + i) * 2 + p) * 256 + l4];
        u32x4 Bd[2];
        Bd[0] = t == 0 ? (u32x4){own[0], own[1], oth[0], oth[1]} : (u32x4){oth[0], oth[1], own[0], own[1]};
        Bd[1] = t == 0 ? (u32x4){own[2], own[3], oth[2], oth[3]} : (u32x4){oth[2], oth[3], own[2], own[3]};
        // ---- project 1x1, K = this group, this wave's half of the output tiles; between its matrix instructions the next group's
        //      expand operands are requested: PRE0 units in front, then one per output tile, into the registers that tile's fragments leave ----
#pragma unroll
        for (int i = 0; i <= MTW; ++i) {
            if constexpr (HASNEXT) {
#pragma unroll
                for (int u = 0; u < kLb4PreUnits; ++u) {
                    const int at = u < PRE0 ? 0 : (u - PRE0 + LAG < MTW ? u - PRE0 + LAG : MTW);
                    if (at == i) lb4_pre_unit<CP>(pre, Wn, u, t, l4, g4);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            if (i == MTW) break;
            acc[i] = mfmaq(Ap[i][1], Bd[0], acc[i]);
            acc[i] = mfmaq(Ap[i][0], Bd[1], acc[i]);
            acc[i] = mfmaq(Ap[i][0], Bd[0], acc[i]);
            if constexpr (HASNEXT) __builtin_amdgcn_sched_barrier(0);
        }
        lb4_wait_vm<NE2>();                              // this wave's pieces of part P of group G+1 have landed: the next top barrier publishes them
    };
    // the last two groups of the stage load the next stage's first group (none without a next stage)
    constexpr unsigned GB = C::GRP_DW * 4;
    for (int G = gb; G < ge - 2; ++G)
        group(Lb4Tag<C>{}, Lb4Tag<C>{}, G, rs, (unsigned)(G + 1) * GB, rs, (unsigned)(G + 2) * GB);
    if (!PARTIAL || gsl >= 2) group(Lb4Tag<C>{}, Lb4Tag<CN>{}, ge - 2, rs, (unsigned)(ge - 1) * GB, rsn, 0u);
    group(Lb4Tag<CN>{}, Lb4Tag<void>{}, ge - 1, rsn, 0u, rsn, 0u);
    if constexpr (PARTIAL) {                             // raw accumulators of this slice -> [slice][B][16][COUT]
        if (real) {
#pragma unroll
            for (int i = 0; i < MTW; ++i)
                *(f32x4 *)&sa.part[(((size_t)blockIdx.y * B + f) * 16 + n) * COUT + 16 * (t * MTW + i) + g4] = acc[i];
        }
        return;
    }

    // ---- rescale, BN shift, residual: lane (n, g) holds channels 16 mt + 4 g .. + 3 of pixel n.  The last stage stores NHWC; the
    //      others keep the result as the next block's residual and hand it over as B fragments ----
    f32x4 vout[MTW];
#pragma unroll
    for (int i = 0; i < MTW; ++i) {
        const int nch = 16 * (t * MTW + i) + g4;
        const size_t at = ((size_t)fc * 16 + n) * COUT + nch;
        f32x4 v = acc[i] * inv_p + *(const f32x4 *)&p_shift[nch];
        if constexpr (C::RES) {
            if (FIRST) v += *(const f32x4 *)&X[at];
            else v += vres[i];
        }
        if (!HANDOFF && real) *(f32x4 *)&Y[at] = v;
        vout[i] = v;
    }
    if constexpr (HANDOFF) {
        static_assert(CN::CIN == COUT && MTW == 5, "the next block takes this block's output: five output tiles per wave");
        unsigned *HO = smem + GRPL;                      // half 1: the last group's weights, no longer read once every wave is here (no load is in flight: vmcnt(0) above)
        lb4_barrier();
#pragma unroll
        for (int i = 0; i < MTW; ++i) {
            vres[i] = vout[i];
            // channels 16 mt + 4 g .. + 3 of pixel n: k32 step mt >> 1, lane group 2 (mt & 1) + (g >> 1), dwords 2 (g & 1), + 1
            const int mt = t * MTW + i, kc = mt >> 1, lt = (2 * (mt & 1) + (g >> 1)) * 16 + n, dw = 2 * (g & 1);
            const f32x4 v = real ? vout[i] * 16.0f : (f32x4){0.f, 0.f, 0.f, 0.f};
            unsigned a0, b0, a1, b1;
            split2q(v[0], v[1], a0, b0);
            split2q(v[2], v[3], a1, b1);
            *(u32x2 *)&HO[((fl * KE + kc) * 2 + 0) * 256 + lt * 4 + dw] = (u32x2){a0, a1};
            *(u32x2 *)&HO[((fl * KE + kc) * 2 + 1) * 256 + lt * 4 + dw] = (u32x2){b0, b1};
        }
        lb4_barrier();
#pragma unroll
        for (int kc = 0; kc < KE; ++kc)
#pragma unroll
            for (int p = 0; p < 2; ++p) Xr[kc][p] = *(const u32x4 *)&HO[((fl * KE + kc) * 2 + p) * 256 + l4];
        // (half 1 is loaded into during the next block's first group, behind that group's top barrier: every wave has these reads back by then)
    }
}

// units of the next group's expand operands requested in front of the project's first matrix instruction (the rest: one per output tile)
// (round 7 took the most that compiled without a spill beside the 24-32 staging registers of the weight copy: the single 160-channel block all
// ten, the chain's 160-channel stages four; the 320-channel stage starts behind its second output tile -- each tile frees eight registers.
// Round 8, with those registers free: the chain at 0 / 2 / 4 / 5 / 6 / 7 / 8 units up front = 131.5 / 128.3 / 127.7 / 127.8 / 127.5 / 127.8 /
// 127.9 us, and ten +1.7 us against four on another box -- flat from two to eight, so the depths stay; two units up front for the
// 320-channel stage spill in its sliced instantiation: docs/history.md, round 8)
constexpr int kPre0Q15 = 10, kPre0Q15C = 4, kPre0Q17 = 0, kLagQ15 = 1, kLagQ15C = 1, kLagQ17 = 2;

template <class C, bool PARTIAL = false>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2)))
void fused_block_lb4_kernel(Lb4StageArgs sa, int B) {
    __shared__ __attribute__((aligned(16))) unsigned smem[C::LDS_DW];
    u32x4 Xr[5][2];
    f32x4 vres[5];
    Lb4Pre pre;
    lb4_stage<C, void, true, C::GRP_DW, PARTIAL, C::MTW == 5 ? kPre0Q15 : kPre0Q17, C::MTW == 5 ? kLagQ15 : kLagQ17>(smem, sa, nullptr, B, Xr, vres, pre);
}

// y = (slice 0 + slice 1 + ... in this order) / (16 Sp) + BN shift (+ x): one thread per four channels of a pixel
template <class C>
__global__ __launch_bounds__(256) void lb4_reduce_kernel(const float *__restrict__ part, int S, const unsigned *__restrict__ Glb,
                                                         const float *__restrict__ p_shift, const float *__restrict__ X,
                                                         float *__restrict__ Y, int B) {
    constexpr int C4 = C::COUT / 4;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x, total = (long)B * 16 * C4;
    if (idx >= total) return;
    const int c4 = (int)(idx % C4);
    const float inv_p = reinterpret_cast<const float *>(Glb + C::WE_DW + C::WP_DW)[11 * 32 + 1];
    f32x4 a = *(const f32x4 *)&part[(size_t)idx * 4];
    for (int sl = 1; sl < S; ++sl) a += *(const f32x4 *)&part[((size_t)sl * total + idx) * 4];
    f32x4 v = a * inv_p + *(const f32x4 *)&p_shift[4 * c4];
    if (C::RES) v += *(const f32x4 *)&X[(size_t)idx * 4];
    *(f32x4 *)&Y[(size_t)idx * 4] = v;
}

using Q15 = Lb4Cfg<160, 960, 160, true>;      // features.15, 16
using Q17 = Lb4Cfg<160, 960, 320, false>;     // features.17

// features.15, 16, 17 of four faces in one launch
constexpr int kChain4Grp = Q17::GRP_DW > Q15::GRP_DW ? Q17::GRP_DW : Q15::GRP_DW;
constexpr int kChain4LdsDw = 2 * kChain4Grp + Q15::XCH_DW;
static_assert(kChain4LdsDw * 4 <= 160 * 1024 && 4 * 5 * 2 * 256 <= kChain4Grp, "LDS budget; the handed-over fragments of four faces fit one buffer half");
struct Lb4ChainArgs { Lb4StageArgs s[3]; };

// No L2 warm-up of the three weight runs at kernel start (syn_internal.h l2_touch), although the same touch gains 4.5 us in the features.7-14
// chain: this kernel's groups are not paced by where the weight lines come from (round-5 negative, 167.4 against 163.3 us: docs/history.md;
// round 7 took the LDS phases off the group boundary for 7 us of 157, so the LDS was not the whole answer either).
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2)))
void fused_chain_lb4_kernel(Lb4ChainArgs ca, int B) {
    __shared__ __attribute__((aligned(16))) unsigned smem[kChain4LdsDw];
    u32x4 Xr[5][2];
    f32x4 vres[5];
    Lb4Pre pre;
    lb4_stage<Q15, Q15, true, kChain4Grp, false, kPre0Q15C, kLagQ15C>(smem, ca.s[0], ca.s[1].Glb, B, Xr, vres, pre);
    lb4_stage<Q15, Q17, false, kChain4Grp, false, kPre0Q15C, kLagQ15C>(smem, ca.s[1], ca.s[2].Glb, B, Xr, vres, pre);
    lb4_stage<Q17, void, false, kChain4Grp, false, kPre0Q17, kLagQ17>(smem, ca.s[2], nullptr, B, Xr, vres, pre);
}

template <class C>
static void launch_lb4(const FusedBlockArgs &a, int B, hipStream_t s) {
    fused_block_lb4_kernel<C><<<(B + 3) / 4, 512, 0, s>>>(Lb4StageArgs{a.X, a.Glb, a.p_shift, a.Y}, B);
}

// small batches: S slices of the hidden groups per four faces (S divides the 30 groups; >= ~192 workgroups), partial sums in `scratch`
template <class C>
static bool launch_lb4_sliced(const FusedBlockArgs &a, int B, hipStream_t s) {
    if (!a.scratch) return false;
    const int wg = (B + 3) / 4;
    static const int divs[] = {2, 3, 5, 6, 10, 15, 30};
    // the fewest slices that give 192 workgroups (more slices lose: 320 / 480 workgroups cost the landmarks-only step +21 / +18 us at B = 128,
    // +25 / +30 at B = 256 -- every slice streams its own partial tensor through the reduce launch)
    int S = 30;
    for (int d : divs) if (wg * d >= 192) { S = d; break; }
    if ((size_t)S * B * 16 * C::COUT > a.scratch_floats) return false;
    Lb4StageArgs sa{a.X, a.Glb, a.p_shift, a.Y};
    sa.part = a.scratch; sa.g0 = 0; sa.g1 = C::NG / S;
    fused_block_lb4_kernel<C, true><<<dim3(wg, S), 512, 0, s>>>(sa, B);
    const long total = (long)B * 16 * (C::COUT / 4);
    lb4_reduce_kernel<C><<<(int)((total + 255) / 256), 256, 0, s>>>(a.scratch, S, a.Glb, a.p_shift, a.X, a.Y, B);
    return true;
}

// features.17 of a small batch: the slices only -- the tail's staging adds them (head_kernel.hip, SIN).  B < 513: the two-face tails.
bool launch_lb4_sliced17_deferred(const FusedBlockArgs &a, int B, hipStream_t s, HeadSliced *out) {
    static const bool on = test_knob("head_sliced_in", 1) != 0;
    static const int wide_min = (int)test_knob("head_wide_min", 513);
    if (!on || !out || !a.Glb || a.prof || !a.scratch || B >= wide_min || B >= 576) return false;
    using C = Q17;
    const int wg = (B + 3) / 4;
    static const int divs[] = {2, 3, 5, 6, 10, 15, 30};
    int S = 30;
    for (int d : divs) if (wg * d >= 192) { S = d; break; }
    // only with two or three slices (>= 253 faces): the tail's staging pays a round of loads per pair of slices -- landmarks-only step, deferred against
    // the reduce launch (ms): B = 512 0.610 / 0.616, 256 0.3744 / 0.3773, 128 (six slices) 0.2837 / 0.2845, 64 0.2575 / 0.2567, 1 (thirty) 0.2167 / 0.2068
    if (S > 3) return false;
    if ((size_t)S * B * 16 * C::COUT > a.scratch_floats) return false;
    Lb4StageArgs sa{a.X, a.Glb, a.p_shift, a.Y};
    sa.part = a.scratch; sa.g0 = 0; sa.g1 = C::NG / S;
    fused_block_lb4_kernel<C, true><<<dim3(wg, S), 512, 0, s>>>(sa, B);
    *out = HeadSliced{a.scratch, S, reinterpret_cast<const float *>(a.Glb + C::WE_DW + C::WP_DW) + 11 * 32 + 1, a.p_shift};
    return true;
}

static int lb4_min_batch() {
    constexpr int min_b = 576;     // fewer faces: hidden-sliced (B = 512: 123 us for the three blocks, 640: 209; the chain: 167 whatever the batch up to 1024)
    return min_b;
}

// a[i] = the arguments of features.(15 + i); false: launch them one by one
bool launch_fused_chain_lb4(const FusedBlockArgs *a, int B, hipStream_t s) {
    static const int chain = (int)test_knob("lb4_chain", 1);
    if (!chain || B < lb4_min_batch()) return false;
    Lb4ChainArgs ca;
    for (int i = 0; i < 3; ++i) {
        if (!a[i].Glb || a[i].prof) return false;
        ca.s[i] = Lb4StageArgs{a[i].X, a[i].Glb, a[i].p_shift, a[i].Y};
    }
    fused_chain_lb4_kernel<<<(B + 3) / 4, 512, 0, s>>>(ca, B);
    return true;
}

bool launch_fused_block_lb4(int feature, const FusedBlockArgs &a, int B, hipStream_t s) {
    if (!a.Glb || a.prof) return false;
    if (B < lb4_min_batch()) {
        // (round 4: hidden-sliced from ONE face on -- thirty one-group workgroups per face quad and a reduce launch take ~15 us per block
        // where the tiled kernel's own sliced schedule, the choice below 32 faces until then, took 43-45: B = 1 0.333 -> ms)
        switch (feature) {
            case 15: case 16: return launch_lb4_sliced<Q15>(a, B, s);
            case 17: return launch_lb4_sliced<Q17>(a, B, s);
            default: return false;
        }
    }
    switch (feature) {
        case 15: case 16: launch_lb4<Q15>(a, B, s); return true;
        case 17: launch_lb4<Q17>(a, B, s); return true;
        default: return false;
    }
}

}  // namespace syn
