// Internal launcher interface between the C-ABI host code (synergy_abi.hip) and the
// gfx950 kernels (backbone_kernels.hip, recon_kernels.hip).  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

struct syn_train_record;                    // include/synergy_hip.h

namespace syn {

#ifdef __HIPCC__
// L2 warm-up ("touch") of a weight run a kernel is going to stream later (round 5).  The kernels of features.7-17 and the head walk 1.6-4 MB of
// weight fragments group by group, fetched ONE group (~1.5 us) ahead; every forward finds them cold (1.4 GB of activations went through
// the 4 MB L2 of each XCD since the last one), so the first CU of an XCD to reach a group pays a miss into the Infinity Cache / HBM of
// about that long, and the CUs of an XCD -- started together -- all wait for the same line fills: timing-only builds of the features.15-17
// chain without its weight fetch ran 21 of 155 us faster (gpurun_out/r5c2).  Here every thread of the launch issues one dword load per
// 128-byte line of its share of the run, long before the run is needed: the misses overlap each other instead of standing in 90 groups.
//   gi / nth: this thread's index among, and the number of, the threads of the launch that run on ITS XCD (workgroup b runs on XCD b % 8).
//   sink: ONE register that receives every touched dword (never read).  It must stay allocated until the loads have returned, which is
//   what l2_touch_done() at the end of the kernel is for.  The loads are inline assembly on purpose: the compiler's wait-count
//   bookkeeping does not know them, so no later s_waitcnt is computed FOR them; vector memory returns in order, hence every wait the
//   compiler inserts for a younger load of its own still covers them (waits can only be longer than needed, never too short).
__device__ __forceinline__ void l2_touch(const void *base, unsigned bytes, unsigned gi, unsigned nth, unsigned &sink) {
    for (unsigned ofs = gi * 128u; ofs < bytes; ofs += nth * 128u) {
        const char *p = static_cast<const char *>(base) + ofs;
        asm volatile("global_load_dword %0, %1, off" : "+v"(sink) : "v"(p) : "memory");
    }
}
__device__ __forceinline__ void l2_touch_done(unsigned &sink) { asm volatile("s_waitcnt vmcnt(0)" : "+v"(sink) :: "memory"); }
#endif

// Test / A-B knobs of the launchers (never needed in production: every default is the measured best).  ONE environment variable,
//   SYNERGY_HIP_TEST_KNOBS = "name=value,name=value,..."   (integers; 0x.. hexadecimal accepted)
// read once per process (synergy_abi.hip); rounds 2-5 had 18 separate SYN_* variables.  Names: lb_chain, lb4_chain, small_f7, head_sliced_in,
// head_wide_min, f16_pair56, rm_pair56, rm_pair34, rm_band2, rm_band3, stem_band, ablate_stem, recon_no_pk, recon_pk_wpg, recon_wgs, recon_prof,
// lt_stage, lt_glds, resnet_exact_mask, wgrad_pass, wgrad_chunk, train_rows.
long long test_knob(const char *name, long long dflt);
bool test_knob_set(const char *name);

constexpr int kImg = 120;           // utils/params.py:34
constexpr int kParam = 62;
constexpr int kPool = 1280;
constexpr int kBasisK = 52;         // 40 shape + 10 expression + 1 (mean u, alpha = 1) + 1 zero pad
constexpr int kVertTile = 32;        // vertices per reconstruction tile (one 32x32 MFMA column block)
// Element k of basis column j (a vertex of the tile) inside one (tile, coordinate) block of kBasisK x 32 floats of the exact-fp32 tiles
// (recon_kernels.hip recon_kernel / lmk_pose_kernel): k = 8 t + 4 h + s < 48 at t 256 + (32 h + j) 4 + s, the tail k = 48 + 2 h + s behind
// them (k = 50: the mean shape, coefficient 1; k = 51: zero pad).  Readers outside recon_kernels.hip go through this.
constexpr int lmk_tile_offset(int j, int k) {
    return k < 48 ? (k >> 3) * 256 + (32 * ((k >> 2) & 1) + j) * 4 + (k & 3) : 6 * 256 + (32 * ((k - 48) >> 1) + j) * 2 + ((k - 48) & 1);
}

// ---- backbone ---------------------------------------------------------------------
// Activations are NHWC fp32: act[b][y][x][c].

// 3x3 stride-2 stem conv + BN scale/shift + ReLU6: NCHW fp32 (or HWC uint8) -> NHWC [B,60,60,32].
void launch_stem(const float *img_nchw, const uint8_t *img_hwc_u8, const float *w27x32,
                 const float *scale, const float *shift, float *out, int B, hipStream_t s);

// Pointwise 1x1 conv as an fp32-MFMA GEMM with fused BN scale/shift (+ReLU6) (+residual):
//   C[m][n] = epi(sum_k A[m][k] * W[n][k]),  A [M,K], W [Npad,Kpad] zero padded, C [M,N].
void launch_pointwise(const float *A, const float *W, const float *scale, const float *shift,
                      const float *residual, float *C, int M, int K, int Kpad, int N,
                      int relu6, hipStream_t s);

// Depthwise 3x3 (pad 1, stride 1|2) + BN scale/shift + ReLU6, NHWC.
void launch_depthwise(const float *in, const float *w9xC, const float *scale, const float *shift,
                      float *out, int B, int Hin, int Hout, int C, int stride, hipStream_t s);

// Global average pool over 4x4 + the three linear heads (one [62,1280] GEMV per face).
void launch_pool_fc(const float *feat /*[B,16,1280]*/, const float *Wfc /*[64,1280]*/,
                    const float *bias /*[64]*/, float *param /*[B,62]*/, float *pool /*nullable*/,
                    int B, hipStream_t s);

// Fused inverted-residual block (expand 1x1 -> dw 3x3 -> project 1x1 [+ residual]) for
// .features[2..17]; weights in MFMA lane order (see fused_block.hip).  Returns false if `feature`
// has no fused configuration.
struct FusedBlockArgs {
    const float *X;                                   // block input  NHWC
    const float *We, *e_scale, *e_shift;              // expand: Wpk[HID/16][CINP/16][64][4], [HID], [HID]
    const float *Wd, *d_scale, *d_shift;              // depthwise: [9][HID], [HID], [HID]
    const float *Wp, *p_scale, *p_shift;              // project: Wpk[COUTP/16][HID/16][64][4], [COUTP], [COUTP]
    float *Y;                                         // block output NHWC
    unsigned long long *prof = nullptr;               // debug: 8 device counters (per-stage s_memtime sums)
    const unsigned *We3 = nullptr, *Wp3 = nullptr;    // split weights: fp16 x2 for features.5-17 (fused_block_f16.hip), bf16 x3 for features.2-4 (fused_block_early.hip), or null
    const float *scl_e = nullptr, *scl_p = nullptr;   // features.5-17: {S, 1/S, 6 S} of the expand / project weights (device)
    const unsigned *Arm_e = nullptr, *Arm_p = nullptr;  // features.2-4: weight fragments of the row-marching kernel (fused_block_rm.hip), or null
    const unsigned *Alb_p = nullptr;                  // features.8-13: project fragments of the register-resident kernel (fused_block_lb.hip), or null
    const unsigned *Alb_e = nullptr;                  // ... its expand fragments
    const float *Tlb = nullptr;                       // ... and its per-group constants table
    const unsigned *Glb = nullptr;                    // features.15-17: per-group runs of fused_block_lb4.hip, or null
    float *scratch = nullptr;                         // workspace for schedules that keep partial sums (hidden-sliced small batches), or null
    size_t scratch_floats = 0;
};
bool launch_fused_block(int feature, const FusedBlockArgs &a, int B, hipStream_t s);
// early blocks (features.2-4) on the bf16 matrix pipe (fused_block_early.hip).  Their hidden width is walked in chunks of
// early_block_hc(HID) channels, each zero padded to a multiple of 32 in the project GEMM's K: the host packs Wp3 that way.
constexpr int early_block_hc(int hid) { return hid % 32 == 0 ? 32 : 48; }
bool launch_fused_block_early(int feature, const FusedBlockArgs &a, int B, hipStream_t s);
// early blocks, row-marching schedule (fused_block_rm.hip): hidden activations stay in registers, one wave per 32 hidden channels.
// Weight fragments for v_mfma_f32_32x32x16_f16, two fp16 pieces per weight (scaled by the layer's power of two, scl_e / scl_p above),
// lane (i = l&31, hh = l>>5) holds 8 K slots, [group][k16 step][piece 2][lane 64][4 dwords]:
//   expand  Arm_e: row i = hidden channel 32g + i, slot e of step s = input channel 16s + 8hh + e        (ceil(CIN/16) steps)
//   project Arm_p: row i = output channel i,       slot e of step s = hidden channel 32g + 16s + 8(e>>2) + 4hh + (e&3)   (2 steps)
// -- the project K order is the register order in which the expand / depthwise stage leaves a lane's 16 channels.
constexpr int rm_expand_dwords(int cin, int hid) { return ((hid + 31) / 32) * ((cin + 15) / 16) * 512; }
constexpr int rm_project_dwords(int hid) { return ((hid + 31) / 32) * 2 * 512; }
bool launch_fused_block_rm(int feature, const FusedBlockArgs &a, int B, hipStream_t s);
// features.3 + 4 / features.5 + 6 (first = 3 | 5) in ONE launch of the row-marching kernel; false: not applicable (launch them one by one)
bool launch_fused_pair_rm(int first, const FusedBlockArgs &a, const FusedBlockArgs &b, int B, hipStream_t s);
// features.5 + 6 of a small batch (<= 256 faces) in ONE launch of the whole-image tiled kernel (fused_block_f16.hip); false: not applicable
bool launch_fused_pair_f16(const FusedBlockArgs &a5, const FusedBlockArgs &a6, int B, hipStream_t s);
// 8x8 blocks (features.8-13), register-resident schedule (fused_block_lb.hip), both GEMMs on v_mfma_f32_16x16x32_f16 with every
// operand as TWO fp16 pieces (x = a + b, 22 significant bits; three products a a, a b, b a) and power-of-two operand scaling
// (synergy_abi.hip pack_backbone_mbv2).  Fragments [..][piece 2][lane 64][4 dwords], lane (m = l&15, kg = l>>4):
//   Alb_e [hidden tile HID/16][k32 step CIN/32]: row = hidden channel 16 nt + m, K slot e = input channel 32 kc + 8 kg + e
//   Alb_p [group HID/32][out tile COUT/16]:      row = output channel 16 mt + m, K slot e = hidden channel 32 G + (e < 4 ? 4 kg + e : 16 + 4 kg + e - 4)
//     -- the order in which the expand / depthwise stage leaves a lane group's eight channels;
//   Tlb [group][12][32] floats: rows 0-8 depthwise filter / Se (tap-major), 9: 16 x depthwise BN shift, 10: 16 Se x expand BN shift,
//     row 11 of group 0: {96 Se, 1 / (16 Sp)}.
constexpr int lb_project_dwords(int hid, int cout) { return (hid / 32) * (cout / 16) * 512; }
constexpr int lb_expand_dwords(int cin, int hid) { return (hid / 16) * (cin / 32) * 512; }
constexpr int lb_table_floats(int hid) { return (hid / 32) * 12 * 32; }
bool launch_fused_block_lb(int feature, const FusedBlockArgs &a, int B, hipStream_t s);
// features.first .. first + n - 1 of every face in ONE launch (a[i]: features.(first + i)).  lb_chain_mode: 3 = features.7-14,
// 2 = features.8-14, 1 = features.8-13, 0 = batch too small / SYN_LB_CHAIN=0 (launch them one by one)
int lb_chain_mode(int B, bool small = true);       // small: batches below the chain threshold may take the one-face-per-workgroup chain (features.8-14, mode 2)
bool launch_fused_chain_lb(const FusedBlockArgs *a, int first, int n_blocks, int B, hipStream_t s);
// 4x4 blocks (features.15-17), fused_block_lb4.hip: the same fragments and constants, but one contiguous run per hidden group
// Glb [group HID/32]: Alb_e fragments of the group's two hidden tiles [tile 2][k32 step][piece 2][64][4] | Alb_p fragments
// [out tile][piece 2][64][4] | Tlb rows [12][32] floats + 128 floats of padding  -- what one LDS-DMA burst copies.
constexpr int lb4_group_dwords(int cin, int cout) { return (2 * (cin / 32) * 512 + (cout / 16) * 512 + 512 + 2047) / 2048 * 2048; }     // padded to 8 KB
bool launch_fused_block_lb4(int feature, const FusedBlockArgs &a, int B, hipStream_t s);
// features.15-17 of every face in ONE launch (a[i]: features.(15 + i)); false = not applicable, launch them one by one
bool launch_fused_chain_lb4(const FusedBlockArgs *a, int B, hipStream_t s);
// same block with both GEMMs on the bf16 matrix pipe through the exact 3-way operand split (features.5-17)
bool launch_fused_block_f16(int feature, const FusedBlockArgs &a, int B, hipStream_t s);

// features.0 + features.1 fused (stem_block1.hip): image -> NHWC [B,60,60,16].
void launch_stem_block1(const float *img_nchw, const uint8_t *img_hwc_u8, const float *w0, const unsigned *w0b3, const float *s0,
                        const float *b0, const float *wd, const float *sd, const float *bd, const float *wp_pk,
                        const float *sp, const float *bp, float *Y, int B, hipStream_t s);

// features.0 + features.1 from uint8 crops, row-marching schedule (stem_rm.hip).  As3: stem filter / 128, scaled by the power of
// two S and split into two fp16 pieces, as fragments of v_mfma_f32_32x32x16_f16, [k16 step 2][piece 2][lane 64][4 dwords], lane
// (i = stem channel, hh = l>>5) K slot q = 8s + e:
//   hh = 0: q < 9 -> tap (ky 0, m = q), 9 <= q < 14 -> (ky 1, m = q - 9);   hh = 1: q < 9 -> (ky 2, m = q), 9 <= q < 13 -> (ky 1, m = q - 4)
//   with m = 3*kx + ci (the byte order of a pixel triple in the HWC image); the other slots are zero.
// s_shift [32]: BN shift - 255/256 * sum of the (scaled) filter, then {S, 1/S, 6 S}; Ap3: the 32->16 projection in rm_project order
// (1 group), scl_p its scales.
constexpr int rm_stem_set_dwords() { return 3 * 2 * 256 + 32 + 4; }      // fragments [3][2][64][4] | shift [32] | {S, 1/S, 6 S, -}
constexpr int rm_stem_dwords() { return 2 * rm_stem_set_dwords(); }      // the uint8 set (filter / 128, shift with the folded -255/256 sum) | the fp32 set (plain)
bool launch_stem_rm(const uint8_t *img8, const unsigned *As3, const float *s_shift, const float *Wd, const float *d_shift,
                    const unsigned *Ap3, const float *p_shift, const float *scl_p, float *Y, int B, hipStream_t s);
// the same march for normalised fp32 NCHW crops [B,3,120,120] (forward_test): As3 / s_shift = the second constant set
bool launch_stem_rm_f32(const float *img, const unsigned *As3, const float *s_shift, const float *Wd, const float *d_shift,
                        const unsigned *Ap3, const float *p_shift, const float *scl_p, float *Y, int B, hipStream_t s);

// features.18 + global average pool + the three heads fused (head_kernel.hip): NHWC [B,4,4,320] -> param [B,62].
void launch_head(const float *X, const float *Wpk /*[80][20][64][4]*/, const float *scale, const float *shift,
                 const float *Wfc /*[64,1280]*/, const float *bfc, float *param, float *pool /*nullable*/, int B,
                 hipStream_t s);

// same tail with the GEMM on the bf16 matrix pipe via an exact 3-way bf16 split of fp32 operands (head_kernel.hip)
// features.17's output still as the hidden-slice partial sums of the small-batch schedule (fused_block_lb4.hip): the tail adds them while it
// stages its input tile -- lb4_reduce_kernel's arithmetic and order -- instead of a reduce launch in front of it (round 5, batches below 513 faces)
struct HeadSliced {
    const float *part;       // [S][B][16][320] raw accumulators
    int S;
    const float *inv_p;      // accumulator -> output scale (one float, device)
    const float *p_shift;    // [320] BN shift of features.17's projection
};
void launch_head_f16x2(const float *X, const unsigned *Wb3 /*[80][10][3][64][4]*/, const float *shift, const float *Wfc,
                        const float *bfc, float *param, float *pool, float *scratch /*[B,1280]*/, int B, hipStream_t s,
                       const HeadSliced *sliced_in = nullptr);
// features.17 hidden-sliced WITHOUT its reduce launch: fills `out` for launch_head_f16x2; false: not applicable (run the block as usual)
bool launch_lb4_sliced17_deferred(const FusedBlockArgs &a, int B, hipStream_t s, HeadSliced *out);

// ---- on-device crop + Lanczos-4 resize (preproc_kernels.hip) ----
void launch_crop_resize(const uint8_t *frame, int H, int W, const int *box, const int *xofs, const short *xcoef,
                        const int *yofs, const short *ycoef, uint8_t *out, int B, hipStream_t s,
                        const long long *foff = nullptr, const int *fdim = nullptr, const int *fidx = nullptr);   // foff: faces of several frames (frame + foff[fidx[b]], fdim[2 f] x fdim[2 f + 1])

// ---- detections -> per-face crop tables on the device (face_tables.hip; the arithmetic is face_tables.h) ----
void launch_lanczos4_tables(const int *sides, int n, int *ofs, short *coef, hipStream_t s);
void launch_face_tables(const float *dets, int n, float *roi, int *box, int *xofs, short *xcoef, int *yofs, short *ycoef, int *status,
                        hipStream_t s);
void launch_compact_detections(const float *dets, const int *counts, const int *order, int N, int K, float thres, float *rows,
                               int *face_frame, int *frame_faces, hipStream_t s);       // one workgroup

// ---- ResNet-50 variant (resnet_kernels.hip) ----
// implicit-GEMM conv, NHWC: W [Npad][KH*KW*Cin] (tap-major), act 0 none / 1 ReLU after the optional residual add
// ResNet-50 activation formats (resnet_kernels.hip "pair format"): inside an fp16 x2 forward every tensor a convolution consumes is stored by
// its producer as the two fp16 pieces of the consumer's MFMA operands ([pixel][32-channel chunk][32 high halves | 32 low halves]); `fmt` is a
// bit set: kFmtOutPair = the output is written in that format, kFmtResPair = the residual is read in it (else fp32 NHWC).
constexpr int kFmtOutPair = 1, kFmtResPair = 2;
// exact fp32-MFMA convolution; in_pair: the input is in the pair format (an fp16 x2 forward), else fp32.  N % 64 == 0.
void launch_conv(const float *in, const float *W, const float *scale, const float *shift, const float *residual, float *out,
                 int B, int Hin, int Hout, int Cin, int N, int KH, int KW, int stride, int pad, int act, hipStream_t s,
                 float *stat = nullptr /* range-guard slot of the output, see launch_conv_f16x2 */, int in_pair = 0, int fmt = 0);
// same conv on the fp16 matrix pipe (two-piece operand split, three products): W3 [N/16][taps*Cin/32][2][64][4] dwords, output channels in pair order,
// Cin % 64 == 0, N % 64 == 0; the input is in the pair format
// stat (nullable): one float of the per-forward range-guard array -- max |output| is folded into it (resnet_kernels.hip range_note)
void launch_conv_f16x2(const float *in, const unsigned *W3, const float *scale, const float *shift, const float *residual,
                     float *out, int B, int Hin, int Hout, int Cin, int N, int KH, int KW, int stride, int pad, int act,
                     hipStream_t s, float *stat = nullptr, int lt = 0 /* 1: the LDS-tiled kernel where its shape fits (N % 128 == 0, M >= 4096); 2: ... 128-pixel tiles only */,
                     int fmt = kFmtOutPair);
// window of a tensor's max |x| inside which the fp16 x2 split of an UNSCALED activation keeps >= 15 bits relative to that maximum:
// above kRangeHi v_cvt_pkrtz_f16_f32 saturates, below kRangeLo even the largest element's low piece is a 4-bit subnormal
constexpr float kRangeHi = 6.0e4f, kRangeLo = 9.765625e-4f;      // 2^-10
// layout of the status array: tensor t owns kRangeSub sub-slots, kRangeStride floats (256 B) apart: stat[(t * kRangeSub + sub) * kRangeStride];
// launchers receive the tensor's base pointer
constexpr int kRangeSub = 64, kRangeStride = 64;
// conv3 + BN + identity + ReLU of a bottleneck fused with the next bottleneck's conv1 + BN + ReLU (resnet_kernels.hip conv_c3f_kernel).
// W3: conv3's fp16 x2 fragments as launch_conv_f16x2 takes them; W1f: the next conv1's fragments step-major [Cin/32][N1/16][piece 2][lane 64][4 dwords]
// (natural K order: in pair order conv3's accumulators are conv1's operand).  T2 / out / T1n in the pair format, identity in it (res_pair) or fp32.
// false: this (K, N1) combination is not instantiated -- launch the two separately.
// conv2 of the bottleneck in front of the fused launch (round 6, 64-channel bottlenecks = layer 1): see resnet_kernels.hip C2Args
struct C2Args {
    const float *T1 = nullptr;      // conv2 input [B, Hin, Hin, 64], pair format
    const unsigned *W2 = nullptr;   // conv2's fp16 x2 fragments as launch_conv_f16x2 takes them
    const float *scale2 = nullptr, *shift2 = nullptr;
    int Hin = 0, Hout = 0, stride = 1;
    unsigned in_bytes = 0;
    float *stat2 = nullptr;         // range-guard slot of conv2's output
};
bool launch_conv_c3f(const float *T2, const unsigned *W3, const float *scale3, const float *shift3, const float *identity, float *out,
                     const unsigned *W1f, const float *s1 /*device {S, 1/S}*/, const float *scale1, const float *shift1, float *T1n, int M, int K, int N3, int N1,
                     hipStream_t s, float *stat3, float *stat1, int res_pair, const C2Args *c2 = nullptr);
// ... with the block's downsample branch (1x1 conv + BN on the block input X [M, Kd]) evaluated in the same kernel instead of read as identity
// (layer1.0: Kd = 64, stride 1); Wd: the downsample conv's fragments as launch_conv_f16x2 takes them.  false: not this shape.
bool launch_conv_c3f_ds(const float *T2, const unsigned *W3, const float *scale3, const float *shift3, const float *X, const unsigned *Wd,
                        const float *scale_d, const float *shift_d, float *out, const unsigned *W1f, const float *s1, const float *scale1,
                        const float *shift1, float *T1n, int M, int K, int Kd, int N3, int N1, hipStream_t s, float *stat3, float *stat1, const C2Args *c2 = nullptr);
// conv3 + the stride-2 downsample branch of a bottleneck as one GEMM over [T2 ; x] with the BatchNorm scales folded into the weights (resnet_kernels.hip DUAL)
bool launch_conv_dual(const float *a, const float *x, const unsigned *W3d, const float *ones, const float *shift, float *out, int B, int H, int C1,
                      int Hin2, int stride2, int Cin2, int N, int act, hipStream_t s, float *stat, int fmt);
bool conv_c3f_supported(int K, int N3, int N1);
void launch_resnet_stem(const float *img_nchw, const uint8_t *img_hwc_u8, const float *w147x64, const float *scale,
                        const float *shift, float *out /*[B,60,60,64]*/, int B, hipStream_t s);
// 7x7 stem on the fp16 matrix instructions (uint8 crops): As3 [group 2][k16 step 10][piece 2][lane 64][4 dwords], lane (i = channel 32G + i,
// hh) K slot kk = 16s + 8hh + e: kernel row ky = kk / 22, m = kk % 22 (m = 0: don't-care byte, else kx = (m-1)/3, ci = (m-1)%3), kk >= 154
// zero; weights / 128 x S (power of two) as two fp16 pieces; s_shift [64] = BN shift - 255/256 * sum of the scaled filter, then {S, 1/S}
constexpr int rn_stem_dwords() { return 2 * 10 * 2 * 256 + 64 + 4; }
// pool != 0: the 3x3 / 2 max-pool in the epilogue, out = [B,30,30,64] (stat: range-guard slot of the pooled tensor, nullable)
bool launch_resnet_stem_mfma(const uint8_t *img8, const unsigned *As3, const float *s_shift, float *out, int B, hipStream_t s, int pool = 0,
                             float *stat = nullptr, int out_pair = 0 /* pool: the pooled tensor in the pair format */);
void launch_maxpool3x3s2(const float *in, float *out, int B, int Hin, int Hout, int C, hipStream_t s, float *stat = nullptr, int out_pair = 0);
void launch_pool_fc_generic(const float *feat, const float *Wfc, const float *bias, float *param, float *pool, int B, int P,
                            int C, int n_out, int out_stride, hipStream_t s, const float *stat = nullptr, int n_stat = 0,
                            unsigned *guard_word = nullptr /* host-mapped word: set to 1 by a forward the range guard poisoned */);
// Test hook (syn_resnet50_span): which KERNEL VARIANT a launcher of resnet_kernels.hip chose is decided inside the launcher (M, N, the step
// count, the 2 GiB limits, the knobs), so the launcher reports it: while resnet_launch_sink is set (by the hook, for the duration of its
// call, on the calling thread) every launch records 1000 x sink->block + its code (include/synergy_hip.h has the table).  NULL in
// production: one host branch per launch, nothing on the device.
struct LaunchSink {
    int codes[160];
    int n = 0, block = 0;
};
extern thread_local LaunchSink *resnet_launch_sink;
inline void note_launch(int code) {
    if (LaunchSink *k = resnet_launch_sink) {
        if (k->n < 160) k->codes[k->n] = 1000 * k->block + code;
        ++k->n;
    }
}
constexpr int kTagStem = 1, kTagStemMfma = 3, kTagStemMfmaPool = 4, kTagMaxpool = 5, kTagConv = 10 /* + MT 1 / 2 / 4 */, kTagF16x2 = 20 /* + MT */,
              kTagH2s = 30 /* + MT */, kTagLt = 40 /* + 2 (MTW == 4) + frag */, kTagLp = 50 /* + 2 (MTW == 4) + frag */, kTagDual = 60, kTagPoolFc = 90,
              kTagC3f = 100 /* + 10 shape (0: K 64 -> N1 64, 1: K 64 -> N1 128, 2: K 128 -> N1 128) + 4 DS + 2 C2F + (identity in pairs) */;
// the two converters of the hook: fp32 NHWC [M][C] <-> the pair format (C % 32 == 0); hi + lo is exact, so the way out loses nothing
void launch_pair_from_f32(const float *in, float *out, size_t M, int C, hipStream_t s);
void launch_f32_from_pair(const float *in, float *out, size_t M, int C, hipStream_t s);

// ---- MobileNetV1 variants (mobilenet1_kernels.hip): mobilenet_1 / _05 / _2, every product exact fp32 ----
// 3x3 / 2 stem + BN + ReLU: NCHW fp32 or HWC uint8 crops -> NHWC [B,60,60,C0]; w [27][C0] (row ci*9 + ky*3 + kx), C0 = 16 | 32 | 64
void launch_mb1_stem(const float *img_nchw, const uint8_t *img_hwc_u8, const float *w, const float *scale, const float *shift,
                     float *out, int C0, int B, hipStream_t s);
// one block (depthwise 3x3 pad 1 stride 1|2 + BN + ReLU -> pointwise 1x1 + BN + ReLU) in one launch: X [B,Hin,Hin,K] -> Y [B,Hout,Hout,N];
// Wd [9][K] tap-major, Wp [N][K] row-major; K % 16 == 0, N % 16 == 0
void launch_mb1_block(const float *X, const float *Wd, const float *d_scale, const float *d_shift, const float *Wp,
                      const float *p_scale, const float *p_shift, float *Y, int B, int Hin, int Hout, int K, int N, int stride,
                      hipStream_t s);
// the default schedule runs the fused launches from this many faces on and the per-layer launches below (synergy_abi.hip run_mobilenet1:
// the one batch threshold of this backbone; at 32 faces the fused launches were measured slower, at 128 faster -- DESIGN 5.13)
constexpr int kMb1FusedMinBatch = 128;
int mb1_block_nt(int N);
// the same block as two launches (the per-layer cross-check schedule)
void launch_mb1_depthwise(const float *in, const float *w9xC, const float *scale, const float *shift, float *out, int B, int Hin,
                          int Hout, int C, int stride, hipStream_t s);
void launch_mb1_pointwise(const float *A, const float *W, const float *scale, const float *shift, float *C, int M, int K, int N,
                          hipStream_t s);

// ---- GhostNet (ghostnet_kernels.hip): every product exact fp32; all pitches, offsets, K and N are multiples of 4 ----
// C[m][n] = act(scale[n] * sum_k A[m][k] gate[m / HW][k] W[n][k] + shift[n]); A rows of pitch lda, C rows of pitch ldc (pass C + offset to
// write a channel slice); scale NULL = 1 (a convolution with a bias); gate NULL = none; act 0 none | 1 ReLU | 2 hard sigmoid
void launch_gn_pointwise(const float *A, int lda, const float *W, const float *scale, const float *shift, const float *gate, int HW,
                         float *C, int ldc, int M, int K, int N, int act, hipStream_t s);
// depthwise ks x ks (3 | 5), stride 1 | 2, pad ks / 2, w [ks*ks][C] tap-major, + BN (+ ReLU) (+ res); in / out / res point at the first
// channel of their slices; pass_out (nullable, stride 1): out-pitched copy of the input pixel + pass_res (nullable, res-pitched)
void launch_gn_depthwise(const float *in, int ldi, const float *w, const float *scale, const float *shift, float *out, int ldo,
                         const float *res, int ldr, float *pass_out, const float *pass_res, int B, int Hin, int Hout, int C, int ks,
                         int stride, int relu, hipStream_t s);
// per-face channel means of in [B][HW] rows of pitch ld -> out [B][C]
void launch_gn_mean(const float *in, int ld, float *out, int B, int HW, int C, hipStream_t s);
// a whole GhostModule: X [B][H*H] rows of pitch ldx, K channels (* gate [B][K]) -> Y [B][H*H][2 N1] = primary | cheap (+ res, pitch ldr)
bool gn_ghost_exists(int H);        // H = 15, 8, 4: a whole face fits the LDS tile
constexpr int kGnTwoFacesMinBatch = 1024;      // 8x8 maps: two faces per workgroup from this many faces on, one below
int gn_ghost_faces(int H, int B);   // faces per workgroup of the fused module
void launch_gn_ghost(const float *X, int ldx, const float *gate, const float *Wp, const float *p_scale, const float *p_shift,
                     const float *Wd, const float *d_scale, const float *d_shift, const float *res, int ldr, float *Y, int B, int H,
                     int K, int N1, int relu, hipStream_t s);

// ---- ResNeSt-50 (resnest_kernels.hip): every product exact fp32; K % 16 == 0, N % 32 == 0 ----
// the pixel operand of launch_rs_gemm: a stored tensor | att0 U0 + att1 U1 | its 3x3 / 2 pad-1 average (/ 9) | the 2x2 / 2 ceil-mode
// average of a stored tensor (divisor = samples inside)
enum RsOp { kRsPlain = 0, kRsCombine = 1, kRsAvd = 2, kRsDsPool = 3 };
// stem convolution 1 (3x3 / 2, 3 -> 32) + BN + ReLU -> NHWC [B,60,60,32]: uint8 HWC crops (normalised inside) or fp32 crops, NCHW
// (img_hwc == 0) or HWC; w [27][32] (row ci*9 + ky*3 + kx)
void launch_rs_stem(const float *img, const uint8_t *img_hwc_u8, int img_hwc, const float *w, const float *scale, const float *shift,
                    float *out, int B, hipStream_t s);
// Y [B,Ho,Ho,N] = act(scale * (op . W^T) + shift (+ res [B,Ho,Ho,N])); W [N][K].  kRsPlain: A rows of pitch lda; kRsCombine: A = U
// [B,Ho,Ho,2K]; kRsAvd: A = U [B,Hin,Hin,2K]; kRsDsPool: A = X [B,Hin,Hin,K]; att [B][2K] (combine and avd only).  The three built
// operands go through an LDS tile and need rs_tail_exists(K, N) (K <= 512: the downsample of layer4.0, K = 1024, has no fused launch)
bool rs_tail_exists(int K, int N);
constexpr int kRsTailGroups = 1024;      // the fused tail splits its channels over workgroups until the grid has this many (4 per CU)
void launch_rs_gemm(int op, const float *A, int lda, const float *att, const float *W, const float *scale, const float *shift,
                    const float *res, float *Y, int B, int Hin, int Ho, int K, int N, int relu, hipStream_t s);
// 3x3 / 1 pad 1, `groups` groups, + BN + ReLU: X [B,H,H] rows of pitch ldx (group q reads channels q Cg ..), W [groups Ng][9][Cg]
// tap-major, Y [B,H,H,groups Ng]
void launch_rs_conv3x3(const float *X, int ldx, const float *W, const float *scale, const float *shift, float *Y, int B, int H, int Cg,
                       int Ng, int groups, hipStream_t s);
// the split-attention gate: U [B,HW,2C] -> att [B][2C]; W1t [C][I], s1 / h1 [I] (BN folded with fc1's bias), W2t [I][2C], b2 [2C]
void launch_rs_gate(const float *U, const float *W1t, const float *s1, const float *h1, const float *W2t, const float *b2, float *att,
                    int B, int HW, int C, int I, hipStream_t s);
// the per-layer schedule's stored operands: V = att0 U0 + att1 U1 [B,HW,C]; the avd pool of V; the downsample pool of X
void launch_rs_combine(const float *U, const float *att, float *V, int B, int HW, int C, hipStream_t s);
void launch_rs_avd(const float *V, float *out, int B, int Hin, int Ho, int C, hipStream_t s);
void launch_rs_dspool(const float *X, float *out, int B, int Hin, int Ho, int C, hipStream_t s);

// ---- resnet18 / resnet34 (resnet_basic_kernels.hip): every product exact fp32; C a power of two >= 64, N % 32 == 0 ----
// 3x3 pad 1 stride 1 | 2 + BN (+ res [B,Ho,Ho,N]) (+ ReLU): X [B,Hin,Hin,C], W [N][9][C] tap-major, Y [B,Ho,Ho,N]; taps from global memory
void launch_bb_conv3x3(const float *X, const float *W, const float *scale, const float *shift, const float *res, float *Y, int B, int Hin,
                       int Ho, int C, int N, int stride, int relu, hipStream_t s);
// the 1x1 stride-2 downsample + BN: W [N][C]
void launch_bb_down1x1(const float *X, const float *W, const float *scale, const float *shift, float *Y, int B, int Hin, int Ho, int C,
                       int N, hipStream_t s);
// the same convolution from an input band staged in LDS; at stride 2 Wd is required and Yd = BN(downsample), from the centre tap
constexpr size_t kBbLdsBytes = 80 * 1024;      // two workgroups share a CU's 160 KiB
constexpr int kBbLdsGroups = 512;              // the channels are split over workgroups until the grid has this many (2 per CU)
constexpr int kBbFacesMinGroups = 256;         // whole faces per workgroup only once that grid has a workgroup for every CU
struct BbLdsGrid { int faces, rows, nb, gridx, split; size_t lds; };      // whole faces per workgroup (0: bands) | output rows per band, bands per face; workgroups, channel ranges, LDS bytes
BbLdsGrid bb_lds_grid(int B, int Hin, int Ho, int C, int N, int stride);
void launch_bb_conv3x3_lds(const float *X, const float *W, const float *scale, const float *shift, const float *res, float *Y,
                           const float *Wd, const float *dscale, const float *dshift, float *Yd, int B, int Hin, int Ho, int C, int N,
                           int stride, int relu, hipStream_t s);

// ---- reconstruction -----------------------------------------------------------------
// basis: pre-packed per 32-vertex tile in MFMA-operand lane order (see recon_kernels.hip):
//   Bp[tile][coord x|y|z][chunk][lane][4], K = 52: 0..39 shape, 40..49 expression,
//   50 = mean u (alpha 1), 51 = 0;  nvp = n_vert rounded up to 32.
// rec: [B,64] float scratch for the per-face records (alpha[52] | M[9] | T[3]).
void launch_reconstruct(const float *param, const float *mean62, const float *std62,
                        const float *basis, int n_vert, int nvp, const float *roi,
                        int transform, float *out, int pitch /*floats between rows of out, >= n_vert*/, int B, hipStream_t s, float *rec);

// Same contraction on v_mfma_f32_32x32x16_f16 (two fp16 pieces per operand, three partial products).
//   basis3: per (32-vertex tile, coord) kBasisF16 dwords: [k16 step 3][piece 2][lane 64][4 dwords] for k = 0..47
//           (lane (j = l&31 vertex, hh = l>>5) holds k = 16*step + 8*hh + e), column k scaled by its own power of two 2^e_k, then one
//           more [lane 64][4] fragment: a fourth k16 step whose slots carry the split partial products of columns 48, 49 and the
//           mean (recon_prep_f16_kernel).  mean62 / std62 here are the COLUMN-SCALED de-whitening constants (entries 12..61 x 2^-e_k,
//           mean62[62] = 2^-e_u, the coefficient of the scaled mean shape): synergy_abi.hip pack_basis.
//   rec3:   per 32-face tile kRecTileF16 dwords: the alpha pieces (x the face's power of two Sa) in the same lane order (faces), the
//           matching fourth-step fragment, then 32 x 16 fp32 records M[9] / Sa | T[3] | 0 x 4.
constexpr int kBasisF16 = (3 * 2 + 1) * 256;
constexpr int kRecTileF16 = (3 * 2 + 1) * 256 + 32 * 16;
constexpr int kRecFloatsPerFace = 96;       // workspace share per face for the records of either layout (+ kRecSlack in total)
constexpr int kRecSlack = 4096;
void launch_reconstruct_f16(const float *param, const float *mean62, const float *std62, const unsigned *basis3, int n_vert,
                           int nvp, const float *roi, int transform, float *out, int pitch, int pad_writable, int B, hipStream_t s, float *rec3,
                           hipEvent_t *marks = nullptr);

// ---- mesh consumers (render_kernels.hip): Sim3DR.get_normal / RenderPipeline / Sim3DR.rasterize / cv2.addWeighted ----
// vertices: F meshes, planar = 1 -> [F,3,nver] (the layout syn_reconstruct writes), 0 -> [F,nver,3] (the reference's)
void launch_mesh_normals(const float *vertices, const int *tri, const int *adj_off, const int *adj_tri, float *tri_normal,
                         float *normal /*[F,nver,3]*/, unsigned *mm /*[F,6] scratch: per-axis min/max keys*/, int F, int nver,
                         int ntri, int planar, hipStream_t s);
void launch_mesh_lighting(const float *vertices, const float *normal, const unsigned *mm, const float *cfg /*16 floats, device*/,
                          float *light /*[F,nver,3]*/, int F, int nver, int planar, hipStream_t s);
// textured meshes: light computed as above, colours = tex * light (shared != 0: one [nver,3] texture multiplied in place face after
// face, lighting.py:69 through utils/render.py:39-42); light may be NULL
void launch_mesh_lighting_tex(const float *vertices, const float *normal, const unsigned *mm, const float *cfg, float *light,
                              float *tex, int shared, float *colors /*[F,nver,3]*/, int F, int nver, int planar, hipStream_t s);
void launch_uv_colors(const unsigned char *uv_tex /*[T,th,tw,ch]*/, const int *coord_u, const int *coord_v, const int *keep /*nullable*/,
                      float *out /*[T,n,ch]*/, int T, int n, int th, int tw, int ch, int normalize, hipStream_t s);
void launch_gather_vertices(const float *vertices /*[F*3] rows `pitch` apart*/, const int *keep, float *out /*[F,3,n_keep]*/, int F,
                            int n_keep, int pitch, hipStream_t s);
void launch_rasterize(const float *vertices, const int *tri, const float *colors /*[F,nver,c]*/, unsigned long long *zkey /*[h*w]*/,
                      unsigned char *image /*[h,w,c] in place*/, int F, int nver, int ntri, int h, int w, int c, int planar,
                      int reverse, hipStream_t s);
void launch_add_weighted(const unsigned char *a, float alpha, const unsigned char *b, float beta, unsigned char *out, size_t n,
                         hipStream_t s);
// visibility buffers: Sim3DR.rasterize_triangles for F meshes, each into its own [h,w] planes (depth / tri_buf / weight in-out: pixels
// no triangle wins keep the caller's values), vertex visibility from the triangle planes, per-vertex colours sampled from a frame,
// and the UV scatter (inverse of launch_uv_colors; highest vertex index wins a shared texel)
void launch_rasterize_triangles(const float *vertices, const int *tri, unsigned long long *zkey /*[F,h,w] scratch*/, float *depth /*[F,h,w]*/,
                                int *tri_buf /*[F,h,w]*/, float *weight /*[F,h,w,3]*/, int F, int nver, int ntri, int h, int w, int planar,
                                hipStream_t s);
// _render_texture_core for F meshes: image / depth in-out, [F,h,w,c] / [F,h,w] or, shared, ONE [h,w,c] / [h,w] all faces compete in;
// texture [T,th,tw,tc] float or uint8 (tex_per_face: T = F, else 1), image float or uint8; zkey [shared ? 1 : F, h, w] scratch
void launch_render_texture(const float *vertices, const int *tri, const int *tex_tri, const float *tex_coords /*[tex_nver,3]*/,
                           const void *texture, int tex_u8, int tex_per_face, int th, int tw, int tc, int mapping, unsigned long long *zkey,
                           void *image, int image_u8, float *depth, int F, int nver, int ntri, int h, int w, int c, int planar, int shared,
                           hipStream_t s);
void launch_vertex_visibility(const int *tri_buf /*[F,h,w]*/, const int *tri, unsigned char *visible /*[F,nver], zeroed here*/, int F,
                              int nver, int ntri, int h, int w, hipStream_t s);
void launch_sample_vertex_colors(const float *vertices, const unsigned char *image /*[h,w,ch]*/, float *out /*[F,nver,ch]*/, int F, int nver,
                                 int h, int w, int ch, int planar, int normalize, hipStream_t s);
void launch_uv_scatter(const float *colors /*[F,nver,ch]*/, const unsigned char *visible /*nullable [F,nver]*/, const int *coord_u,
                       const int *coord_v, unsigned *owner /*[F,th,tw] scratch*/, unsigned char *tex /*[F,th,tw,ch]*/,
                       unsigned char *mask /*[F,th,tw]*/, int F, int nver, int th, int tw, int ch, hipStream_t s);

// ---- push-pull completion of UV textures (texture_kernels.hip): three launches for any size and batch ----
// scratch: texture_fill_scratch_bytes(Tout, ...) bytes, Tout = 1 with merge else T; out [Tout,th,tw,ch]
constexpr int kTextureFillMaxDim = 4096;                        // th, tw beyond it are refused by syn_texture_fill; the kernels' LDS is sized by it
size_t texture_fill_scratch_bytes(int Tout, int th, int tw, int ch);
void launch_texture_fill(const unsigned char *tex /*[T,th,tw,ch]*/, const unsigned char *mask /*[T,th,tw]*/, unsigned *scratch,
                         unsigned char *out, int T, int th, int tw, int ch, int merge, hipStream_t s);

// ---- AFLW2000-3D landmark error (eval_kernels.hip) ----
void launch_nme(const float *fit, const float *gt, const float *roi, float *nme, int N, hipStream_t s);

// ---- FaceBoxes detector (detector_kernels.hip) ----
// N frames of one size per launch (grid y).  Pointers are frame 0's; frame f's scratch (in / out / loc / conf / cand) lies f * fstride
// floats further, its frame, dets [keep_top_k,5], boxes_out / scores_out and counters (n_cand[f], n_out[f]) at their natural strides.
void launch_det_preproc(const unsigned char *frames, int N, int H, int W, float *out, int Ho, int Wo, size_t fstride, hipStream_t s);
void launch_det_conv(const float *in, const float *Wt, const float *shift, float *out, int N, size_t fstride, int Hi, int Wi, int cs_in, int ci0,
                     int Cin, int Ho, int Wo, int cs_out, int co0, int Cout, int K, int stride, int pad, int act, hipStream_t s);
void launch_det_pool(const float *in, float *out, int N, size_t fstride, int Hi, int Wi, int C, int Ho, int Wo, int stride, int is_max,
                     hipStream_t s);
void launch_det_decode(const float *loc, const float *conf, int N, size_t fstride, int P, int Hn, int Wn, int H4, int W4, int H5, int W5, int H6,
                       int W6, float scale, float thr, float *cand, int *n_cand, int max_cand, float *boxes_out, float *scores_out,
                       hipStream_t s);
void launch_det_nms(const float *cand, const int *n_cand, int N, size_t fstride, int max_cand, int top_k, float nms_thr, int keep_top_k,
                    float *dets, int *n_out, hipStream_t s);
int det_sort_capacity();

// ---- synergy refinement: MLP_for / MLP_rev (synergy_kernels.hip) ----
// Weights: row-major [N][K] fp32, N padded to a multiple of 16 (conv9: 3 -> 16, MLP_rev's head: 62 -> 64) and K to a multiple of 16
// (conv1: 3 -> 4, one MFMA step) with zeros; scale / shift per output channel, padded like N (syn_load_synergy).
constexpr int kSynPts = 68;                 // points per face (MLP_for(68) / MLP_rev(68), synergy3DMM.py:82-84)
constexpr int kSynGlobal = 1024;            // width of the max-pooled global feature
constexpr int kSynFaceK = kSynGlobal + kPool + 40 + 10;      // per-face input columns of conv6: global | pool | shape | expr = 2354
constexpr int kSynFaceKpad = (kSynFaceK + 15) / 16 * 16;     // 2368
struct SynTrunkW { const float *W[5], *scale[5], *shift[5]; };                   // conv1 .. conv5
struct SynHeadW {
    const float *W6p, *scale6, *shift6;      // conv6, per-point columns [512][64]
    const float *W7, *scale7, *shift7;       // [256][512]
    const float *W8, *scale8, *shift8;       // [128][256]
    const float *W9, *scale9, *shift9;       // [16][128], rows 3..15 zero
};
// conv1-conv5 + max over a face's 68 points: lmk [B,3,68] -> gf[b * gf_pitch + 0..1023] (and gf2 [B,1024] when given); pf: conv2's
// output [B*68,64] (MLP_for's point features) or null
void launch_syn_trunk(const SynTrunkW &w, const float *lmk, int B, float *pf, float *gf, int gf_pitch, float *gf2, hipStream_t s);
// columns 1024 .. 2367 of X6 [B,2368]: pool | whitened param[12:62] | zeros
void launch_syn_face_concat(const float *pool, const float *param, float *X6, int B, hipStream_t s);
// out[b][n] = sum_k W[n][k] X[b][k] (scale == null) or relu(scale[n] * sum + shift[n]); W [ceil32(N)][Kpad], Kpad % 16 == 0
void launch_syn_face_gemm(const float *X, int ldx, const float *W, int Kpad, const float *scale, const float *shift, float *out, int ldo,
                          int N, int B, hipStream_t s);
// conv6 .. conv9 on the point features + g6 [B,512] (the per-face half of conv6), out = lmk_in + 0.05 res, then the ROI affine if roi
void launch_syn_point_head(const SynHeadW &w, const float *pf, const float *g6, const float *lmk_in, const float *roi, float *out, int B,
                           hipStream_t s);

void launch_pose(const float *param, const float *mean62, const float *std62, const float *roi,
                 double *angles /*nullable together with t3d*/, float *t3d, float *pmat /*nullable [B,3,4]*/, int B, hipStream_t s);
// landmarks + pose in one launch (recon_kernels.hip lmk_pose_kernel): fp32 landmark tiles, plain fp32 multiply-adds
void launch_lmk_pose(const float *param, const float *mean62, const float *std62, const float *basis_lmk, int n_lmk, int nlp, const float *roi,
                     int transform, float *lmk, double *angles, float *t3d, int B, hipStream_t s);

// ---- losses of the training graph's forward + CenterCrop (loss_kernels.hip) ----
// Batch sums are cut into FIXED chunks, one workgroup each, and folded by the workgroup that finishes last (an integer ticket counter,
// zero before the launch and zero again after it): the order of every sum depends on the element count only.
constexpr int kWingChunk = 2048;            // elements per workgroup of wing_loss_kernel
constexpr int kLossFaces = 8;               // faces per workgroup of synergy_losses_kernel
inline unsigned wing_chunks(size_t N) { return (unsigned)((N + kWingChunk - 1) / kWingChunk); }
inline unsigned loss_groups(int B) { return (unsigned)((B + kLossFaces - 1) / kLossFaces); }
// partial: [wing_chunks(N)][2] doubles of scratch; loss: one float
void launch_wing_loss(const float *pred, const float *target, size_t N, float omega, float epsilon, double *partial, unsigned *counter,
                      float *loss, hipStream_t s);
void launch_param_loss(const float *input, const float *target, int B, int mode /*0 normal | 1 only_3dmm*/, float *loss, hipStream_t s);
// partial: [loss_groups(B)][8] doubles of scratch; scalars [2], per_face [3][B], meter nullable [8] doubles
void launch_synergy_losses(const float *param, const float *target, const float *lmk, const float *lmk_gt, const float *lmk_refined,
                           const float *param_rev, int B, double *partial, unsigned *counter, float *scalars, float *per_face, double *meter,
                           hipStream_t s);
void launch_center_crop_u8(const uint8_t *in, uint8_t *out, int B, int H, int W, int C, int margin, hipStream_t s);

// ---- train-time augmentation (augment_kernels.hip): ColorJitter + CenterCrop(train) + Normalize, one workgroup per output face ----
// records: B device records; either output nullable.  The caller has checked 3 H W against SYN_TRAIN_TRANSFORM_MAX_FACE_BYTES.
hipError_t launch_train_transform(const uint8_t *src, int N, int H, int W, const syn_train_record *records, int B, int margin, float mean,
                                  float stdv, float *out_f32, uint8_t *out_u8, hipStream_t s);

// ---- backward of the two loss modules (loss_backward_kernels.hip) ----
// count: [wing_chunks(N) + 1] 64-bit words of scratch (chunk counts, then n); g nullable (1 float: upstream gradient 1); counter as above
void launch_wing_loss_backward(const float *pred, const float *target, size_t N, float omega, float epsilon, const float *g,
                               unsigned long long *count, unsigned *counter, float *d_pred, hipStream_t s);
// g nullable ([B]: ones); d_input / d_target [B,62], either nullable
void launch_param_loss_backward(const float *input, const float *target, int B, int mode, const float *g, float *d_input, float *d_target,
                                hipStream_t s);
void launch_wing_count(const float *pred, const float *target, size_t N, float omega, unsigned long long *count, unsigned *counter, hipStream_t s);

// backward of the whole loss head (loss_backward_kernels.hip head_backward_kernel): one face at a time per workgroup
constexpr int kHeadWs = 176816;             // floats of scratch per workgroup (the kernel's static_assert pins the layout)
constexpr int kHeadGroupsMax = 512;         // faces of one pass of the backward's launches: the images stop growing there, a larger batch takes several passes
constexpr int kHeadFaceFloats = 1024 + 64 + 64 + 64 + 1024 + 512 + 2368;     // per-face vectors between the launches
struct HeadBwdArgs {
    SynTrunkW tf, tr;                        // MLP_for / MLP_rev trunks
    SynHeadW hw;
    const float *W6f, *Wrev, *sc_rev, *sh_rev;
    const float *mean, *stdv, *basis;        // de-whitening constants, fp32 landmark tiles
    const float *param, *target;             // [B,62]
    const float *Lc, *Lgt, *Lr, *pf, *G6;    // what the forward launches left in scratch
    const unsigned long long *n0, *n1;       // elements counted by the two WingLosses
    const float *g_scalars, *g_per_face;     // nullable together: 1 and 1 / B
    float *ws;                               // the workgroups' images, kHeadWs floats each
    float *GFRg, *S2g, *GS2g, *DPARg, *DGFRg, *DG6g, *DX6g;     // per face: [1024] [64] [64] [64] [1024] [512] [kSynFaceKpad]
    float *d_param, *d_pool;
    int B;
    // weight gradients, all three null unless syn_synergy_losses_backward_weights runs the phases: the workgroups' images
    // of UNSCALED masked gradients (kHeadWg floats each) and, per face, MLP_rev's heads' [64] and conv6's per-face half [512]
    float *wg = nullptr, *GS2Ug = nullptr, *DG6Ug = nullptr;
};
// a workgroup's image (float offsets, all multiples of 4; head_backward_kernel and the weight products of loss_wgrad_kernels.hip)
namespace headimg {
constexpr int kP = kSynPts;
constexpr int oA1 = 0, oA3 = oA1 + kP * 64, oA4 = oA3 + kP * 64, oH6 = oA4 + kP * 128, oH7 = oH6 + kP * 512, oH8 = oH7 + kP * 256,
              oB1 = oH8 + kP * 128, oB2 = oB1 + kP * 64, oB3 = oB2 + kP * 64, oB4 = oB3 + kP * 64, oD0 = oB4 + kP * 128, oD1 = oD0 + kP * 512,
              oDA2X = oD1 + kP * 512, oARGF = oDA2X + kP * 64, oARGR = oARGF + 1024, oM9 = oARGR + 1024, oDLR = oM9 + kP * 4,
              oDLC = oDLR + 208, oEnd = oDLC + 208;
static_assert(oEnd == kHeadWs, "kHeadWs");
// the image of unscaled gradients g (ReLU mask applied, before the multiplication by the layer's scale), [68][N] each:
// MLP_rev conv4 .. conv1 | MLP_for conv9 (N = 4, column 3 zero), conv8, conv7, conv6 | MLP_for conv4 .. conv1
constexpr int wR4 = 0, wR3 = wR4 + kP * 128, wR2 = wR3 + kP * 64, wR1 = wR2 + kP * 64, wG9 = wR1 + kP * 64, wG8 = wG9 + kP * 4,
              wG7 = wG8 + kP * 128, wG6 = wG7 + kP * 256, wF4 = wG6 + kP * 512, wF3 = wF4 + kP * 128, wF2 = wF3 + kP * 64, wF1 = wF2 + kP * 64,
              wEnd = wF1 + kP * 64;
}  // namespace headimg
constexpr int kHeadWg = headimg::wEnd;      // 104 720 floats
constexpr int kHeadWgPass = 256;            // default faces per pass of syn_synergy_losses_backward_weights (test knob wgrad_pass)
constexpr int kHeadWgChunk = 4;             // default faces per chunk of the per-point weight products (test knob wgrad_chunk)

// ---- weight gradients of the loss head (loss_wgrad_kernels.hip) ----
// The 17 layers of the FLAT layout (MLP_for conv1 .. conv9, MLP_rev conv1 .. conv5, conv6_1 .. conv6_3): offsets in floats
struct SynFlatLayer { size_t w, bias, bn; int N, K; };      // weight [N][K] | bias [N] | gamma, beta, mean, var [4][N]
constexpr int kSynFlatLayers = 17;
SynFlatLayer syn_flat_layer(int i);
size_t syn_flat_total();
// Accumulators of Gx = sum g (x) x per layer, [pad16(N)][ld] with the sum s of g in column K (conv6's per-face half has none: its s is
// that of the per-point half).  They live in scratch for the length of one call.
struct HeadWgAcc { float *t[2][5], *c6p, *c6f, *c7, *c8, *c9, *rev; float *part; int chunk; };      // part: the chunks' partial tiles of a pass
size_t head_wgrad_acc_floats();
size_t head_wgrad_part_floats(int pass, int chunk);      // partial tiles of the per-point layers for a pass cut into chunks of `chunk` faces
void head_wgrad_acc_carve(float *base, HeadWgAcc &acc);
// the products of one pass (faces [b0, b0 + nb), images in a.ws / a.wg) added to the accumulators in a fixed order; first: start from 0
void launch_head_wgrad_pass(const HeadBwdArgs &a, const HeadWgAcc &acc, const float *X6, int b0, int nb, bool first, hipStream_t s);
// d_flat (every element) from the accumulators and the unfolded flat state on the device
void launch_head_wgrad_final(const HeadWgAcc &acc, const float *flat, float *d_flat, hipStream_t s);
// fold + repack a flat state on the device into the kernel-ready image of syn_load_synergy
struct SynFoldLayer { size_t dstA, dstB, dstScale, dstShift; int ldA, ldB, KA; };    // columns [0, KA) -> dstA, [KA, K) -> dstB
struct SynFoldTable { SynFoldLayer L[kSynFlatLayers]; };
void launch_syn_fold_device(const float *flat, float *blob, const SynFoldTable &t, hipStream_t s);
// phase 0 .. 3 of the walk for faces [b0, b0 + faces), faces <= kHeadGroupsMax (see head_backward_kernel)
void launch_head_backward_phase(int phase, const HeadBwdArgs &a, int b0, int faces, hipStream_t s);
// out[b][k] = sum_n G[b][n] W[n][k], W [N][K] row-major with N % 16 == 0 and K % 32 == 0: one wave per 16 faces x 32 outputs
void launch_face_tgemm(const float *G, int ldg, const float *W, int ldw, int N, float *out, int ldo, int K, int B, hipStream_t s);

// ---- the loss head's forward under BatchNorm batch statistics (loss_train_kernels.hip) ----
constexpr int kSynBnChannels = 2243 + 1406;  // MLP_for bn1 .. bn9 | MLP_rev bn1 .. bn5, bn6_1 .. bn6_3, the FLAT layout's order
constexpr int kTrainRows = 256;             // default rows per block of the statistics' partial sums (test knob train_rows, >= 16)
constexpr int kTrainMaxFaces = 4096;        // the largest batch syn_synergy_losses_train accepts (2.4 GB of scratch)
struct SynTrainArgs {
    const float *Wt[2][5];                   // the trunks' packed RAW weights of syn_load_synergy (conv1: [64][4])
    const float *W6p, *W6f, *W7, *W8, *W9, *Wrev;
    float *flat;                             // the unfolded state: bias, gamma, beta are read, the running statistics written when momentum >= 0
    const float *Lc, *pool, *param;          // crop-space landmarks of param [B,3,68]; the head's inputs
    float *Lr, *S2;                          // out: refined landmarks [B,3,68], MLP_rev's parameters [B,62]
    float *scratch;                          // train_scratch_floats(B) floats
    double *part;                            // train_part_doubles(B, rows) doubles
    float *batch_stats;                      // nullable [2][kSynBnChannels]
    float momentum;
    int B, rows;
};
size_t train_scratch_floats(int B);
size_t train_part_doubles(int B, int rows);
// MLP_for on Lc and MLP_rev on its result, layer by layer, every BatchNorm by the statistics of the batch
void launch_synergy_train_head(const SynTrainArgs &a, hipStream_t s);

}  // namespace syn
