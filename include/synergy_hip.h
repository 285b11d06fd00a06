/*
 * synergy_hip.h -- C ABI of the MI355X (gfx950) implementation of SynergyNet's
 * inference hot path:
 *
 *   crops [B,3,120,120] -> MobileNetV2 -> 62-d 3DMM params -> 68 landmarks,
 *   53215-vertex mesh, head pose.
 *
 * The reference has no FFI layer for this path; its boundary is the Python
 * class synergy3DMM.SynergyNet (reference synergy3DMM.py:70-207).  Each entry
 * point below names the reference method(s) it replaces.  The Python class
 * synergynet_amd.synergy3DMM.SynergyNet binds these symbols with ctypes and
 * keeps the reference's method set (INTEGRATION.md shows the binding).
 *
 * Conventions
 *   - plain C types only; every function returns 0 on success or a negative
 *     syn_status, and syn_last_error() returns a thread-local message;
 *   - all tensor arguments of compute calls are DEVICE pointers owned by the
 *     caller (e.g. torch-ROCm tensor.data_ptr()), fp32, contiguous;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls
 *     are asynchronous on that stream;
 *   - the library owns only its packed constants and its activation workspace;
 *   - one handle per device; calls on one handle are not thread-safe, different
 *     handles are independent.
 */
#ifndef SYNERGY_HIP_H
#define SYNERGY_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct syn_handle syn_handle;

typedef enum {
    SYN_OK = 0,
    SYN_ERR_INVALID = -1,      /* bad argument (NULL pointer, B <= 0, wrong size ...) */
    SYN_ERR_HIP = -2,          /* a HIP runtime call failed; see syn_last_error()     */
    SYN_ERR_NOT_LOADED = -3,   /* compute call before the constants it needs          */
    SYN_ERR_PARAM_LEN = -4     /* 'length of params mismatch' (synergy3DMM.py:126-129) */
} syn_status;

#define SYN_PARAM_DIM 62        /* 12 pose + 40 shape + 10 expression (synergy3DMM.py:30-37) */
#define SYN_POOL_DIM 1280       /* pooled feature (mobilenetv2_backbone.py:179-182)          */
#define SYN_STD_SIZE 120        /* utils/params.py:34                                        */

const char *syn_last_error(void);
int syn_abi_version(void);

/* SynergyNet.__init__ (synergy3DMM.py:70-114): one handle per GPU. */
int syn_create(int device, syn_handle **out);
int syn_destroy(syn_handle *h);

/* ---- constants ------------------------------------------------------------------- */

/* Number of floats syn_load_backbone expects. */
size_t syn_backbone_flat_count(void);

/* load_weights (synergy3DMM.py:156-164) for the I2P.backbone.* part of the state_dict.
 * `flat` is a HOST array: for every conv layer in network order
 *   conv.weight (PyTorch [Cout,Cin/groups,kh,kw] order), bn.weight, bn.bias,
 *   bn.running_mean, bn.running_var
 * then classifier_ori.1.{weight,bias}, classifier_shape.1.{...}, classifier_exp.1.{...}
 * (mobilenetv2_backbone.py:33-74,107-158).  BatchNorm (eval, eps 1e-5) is turned into a
 * per-channel scale/shift and the weights are repacked for the kernels. */
int syn_load_backbone(syn_handle *h, const float *flat, size_t n_floats);

/* Range safety of the fp16 arithmetic.  Every GEMM of the default schedule carries its fp32 operands as two fp16 pieces (22-bit
 * significand, fp32 accumulation); fp16's exponent range is 2^-14 .. 65504, and the reference loads ARBITRARY checkpoints
 * (synergy3DMM.py:156-164).  syn_load_backbone therefore bounds, from the folded constants alone, every tensor that is split at run
 * time (interval arithmetic: hidden activations are in [0,6] after ReLU6, project outputs and residual sums follow from the weights)
 * and checks every packed weight row; a block whose bound does not fit runs the tiled fp16 kernel at input scale 1 or the exact
 * fp32-MFMA kernel instead (csrc/synergy_abi.hip analyze_mbv2_ranges).  The verdict travels with exported constants.
 * syn_numerics_report: one text line per .features[] index into buf (NUL terminated, truncated to n); returns the number of
 * blocks that do NOT run the default kernel (0 = the whole network is inside the fp16 window), or a negative syn_status. */
int syn_numerics_report(syn_handle *h, char *buf, size_t n);

/* Which arithmetic the compute calls of this handle use from now on: 2 (default) fused kernels with fp16x2 operands, 1 fused kernels on
 * the fp32-input MFMA (exact fp32 products: the cross-check and fallback schedule), 0 one fp32 kernel per layer.  Returns the previous
 * value (>= 0) or a negative syn_status.  Lets a caller compare the default schedule with the exact one ON ITS OWN CHECKPOINT AND
 * IMAGES without an oracle (SynergyNet.check_numerics).  Not to be changed while calls are in flight. */
int syn_set_schedule(syn_handle *h, int fusion);

/* Calibration of that verdict on the caller's own crops (uint8 [B,120,120,3] on the device, B <= 256): every block output of the default
 * schedule is compared with the exact fp32-MFMA schedule on this data; a block that differs by more than `tol` (relative to the
 * tensor's maximum; 2e-5 is the natural choice, the schedules agree to ~1e-6) runs the exact kernel from then on, in this handle and
 * in every replica that imports its constants.  Closes the one assumption of the load-time analysis that is not a proof: that the
 * interval bound of a tensor is within 2^8 of its true activations (underflow side).  Returns the number of blocks switched
 * (0 for ResNet-50, which is guarded at run time).  Synchronises; not for use while forwards of this handle are in flight.
 * Scope of the check: the comparison runs block by block at B <= 256, i.e. on the kernels THAT batch size selects (tiled /
 * band-marching early blocks, features.8-13 one block per launch).  The whole-face row-marching kernels of B >= 352 ... 513 and the
 * chain launches use the same operand pieces, scales and range proofs but another summation order; the verdict is taken as valid for
 * them because what it measures -- operand underflow of a block's input and weights -- does not depend on the order of the sum. */
int syn_backbone_calibrate(syn_handle *h, const uint8_t *crops_u8, int B, float tol, void *stream);

/* ResNet-50 (ReLU, no static activation bound): the fp16 convolutions are guarded at RUN time.  Every tensor they split reports
 * max |x| into a per-forward status array; when one leaves [2^-10, 6e4] the head kernel returns NaN for that forward (loud, no host
 * synchronisation).  syn_backbone_range_status synchronises the device, copies the maxima of the last forward (slot 0 = max-pool
 * output, 1 + i = convolution i in state_dict order; unguarded slots read 1) and returns the number of tensors outside the window;
 * with fallback != 0 a violation switches the handle to the exact fp32-MFMA convolutions for all later forwards.  0 for MobileNetV2. */
int syn_backbone_range_status(syn_handle *h, float *layer_max, int max_layers, int fallback);
/* The same switch happens by itself: the head kernel of a poisoned forward also writes a page-locked word of the handle, which the
 * NEXT syn_backbone_forward* reads at its entry (no synchronisation) -- from then on the handle runs the exact convolutions.  A
 * caller that never asks sees one NaN batch (as many as were already in flight), not NaN for ever (reference behaviour being
 * replaced: synergy3DMM.py:156-164 loads any checkpoint and always answers).  syn_backbone_range_events returns how many such
 * automatic or requested switches happened since the weights were loaded (0 | 1); after a switch syn_backbone_range_status
 * reports 0 violations and maxima of 1 (the guard is no longer armed). */
int syn_backbone_range_events(syn_handle *h);

/* BASELINE config 5: the ResNet-50 backbone (reference backbone_nets/resnet_backbone.py:139-254, resnet50 :304-312).
 * `flat` = conv1.weight, bn1.{weight,bias,running_mean,running_var}, then per block of layer1..layer4:
 * conv1, bn1, conv2, bn2, conv3, bn3, [downsample.0, downsample.1], then fc_tex, fc_ori, fc_shape, fc_exp
 * ({weight,bias} each) -- the reference's state_dict order.  After this call syn_backbone_forward*() run ResNet-50
 * and return the first 62 of its 102 outputs (ori 12 | shape 40 | exp 10; the texture head is dropped), which is the
 * adapter the reference's own wrapper would need.  pool = the 2048-d pooled feature. */
size_t syn_resnet50_flat_count(void);
int syn_load_backbone_resnet50(syn_handle *h, const float *flat, size_t n_floats);
double syn_resnet50_flops_per_face(void);

/* The MobileNetV1 backbones (reference backbone_nets/mobilenetv1_backbone.py:47-140; `--arch mobilenet_1` of main_train.py, the
 * default of benchmark_validate.py).  Backbone ids, as in the `arch` word of the constants header:
 *   0 mobilenet_v2 | 1 resnet50 | 2 mobilenet_1 (width 1.0) | 3 mobilenet_05 (0.5) | 4 mobilenet_2 (2.0)
 * (widths 0.25 and 0.75 have 8 / 24-channel layers, no multiple of the 16-wide matrix tile, and are not offered).
 * `flat` = the module's state_dict() order without num_batches_tracked: conv1.weight, bn1.{weight,bias,running_mean,running_var},
 * then per block dw2_1, dw2_2, dw3_1, dw3_2, dw4_1, dw4_2, dw5_1 .. dw5_6, dw6: conv_dw.weight, bn_dw.*, conv_sep.weight, bn_sep.*,
 * then fc_ori, fc_shape, fc_exp, fc_tex {weight, bias}.  BatchNorm is folded on the host (eps 1e-5).  After loading,
 * syn_backbone_forward[_u8] run this network: stem, 13 fused depthwise + pointwise launches, pool + heads, every product exact
 * fp32 (fp32-input MFMA), so syn_numerics_report has nothing to prove and syn_backbone_range_status / _calibrate return 0.
 * They return the first 62 of the 102 outputs (ori 12 | shape 40 | exp 10: the reference's own cat order; the texture head is
 * loaded but never computed); pool = the pooled feature, 1024 x width floats.  SYNERGY_HIP_FUSION / syn_set_schedule(h, .): 2 (default)
 * the fused launches from 128 faces on and one depthwise + one pointwise launch per block below, where those are the faster ones; 1 the
 * fused launches at every batch size; 0 the per-layer launches at every batch size (the cross-check schedule).
 * syn_mobilenet1_flat_count / _flops_per_face return 0 for an id that is not 2, 3 or 4. */
size_t syn_mobilenet1_flat_count(int arch);
double syn_mobilenet1_flops_per_face(int arch);
int syn_load_backbone_mobilenet1(syn_handle *h, int arch, const float *flat, size_t n_floats);

/* The GhostNet backbone (reference backbone_nets/ghostnet_backbone.py:76-266, width 1.0; `--arch ghostnet` of main_train.py).
 * Backbone id 6.  The whole id table:
 *   0 mobilenet_v2 | 1 resnet50 | 2 mobilenet_1 | 3 mobilenet_05 | 4 mobilenet_2 | 5: never assigned | 6 ghostnet
 * `flat` = the module's state_dict() order without num_batches_tracked (synergynet_amd.synergy3DMM.ghostnet_keys): conv_stem.weight, bn1.*,
 * then per bottleneck blocks.S.I: ghost1.{primary_conv.0.weight, primary_conv.1.*, cheap_operation.0.weight, cheap_operation.1.*},
 * [conv_dw.weight, bn_dw.* when stride 2], [se.conv_reduce.{weight,bias}, se.conv_expand.{weight,bias}], ghost2.{...},
 * [shortcut.0.weight, shortcut.1.*, shortcut.2.weight, shortcut.3.* when in != out or stride 2]; blocks.9.0.conv.weight, blocks.9.0.bn1.*,
 * conv_head.{weight,bias}, classifier_ori / _shape / _exp / _texture {weight, bias}.  BatchNorm is folded on the host in fp32 (eps 1e-5).
 * After loading, syn_backbone_forward[_u8] run this network, every product exact fp32 (fp32-input MFMA, fp32 depthwise and SE means):
 * syn_numerics_report has nothing to prove, syn_backbone_range_status / _calibrate return 0.  They return the first 62 of the 102
 * outputs (ori 12 | shape 40 | exp 10; classifier_texture is loaded but never computed); pool = the 1280 outputs of conv_head + ReLU
 * (act2), what the heads consume -- 1280 wide like mobilenet_v2's, so syn_refine_landmarks and the synergy forward accept this arch.
 * SYNERGY_HIP_FUSION / syn_set_schedule(h, .): 0 = one launch per layer (104 launches, the cross-check); 1 = every GhostModule on a
 * 15x15, 8x8 or 4x4 map as one launch (79 launches); 2 (default) = as 1.  syn_ghostnet_flops_per_face = 2 x 45 802 556 MAC, the
 * module with all four heads. */
size_t syn_ghostnet_flat_count(void);
double syn_ghostnet_flops_per_face(void);
int syn_load_backbone_ghostnet(syn_handle *h, const float *flat, size_t n_floats);

/* The ResNeSt-50 backbone (reference backbone_nets/ResNeSt/resnest.py:33-41, resnet.py, splat.py; `--arch resnest50` of main_train.py:
 * radix 2, cardinality 1, deep stem of width 32, avg_down, avd after the split-attention convolution).  Backbone id 8.  The whole id table:
 *   0 mobilenet_v2 | 1 resnet50 | 2 mobilenet_1 | 3 mobilenet_05 | 4 mobilenet_2 | 5: never assigned | 6 ghostnet | 7: never assigned | 8 resnest50
 * `flat` = the module's state_dict() order without num_batches_tracked (synergynet_amd.synergy3DMM.resnest50_keys): conv1.0.weight,
 * conv1.1.*, conv1.3.weight, conv1.4.*, conv1.6.weight, bn1.*, then per bottleneck layerL.I: conv1.weight, bn1.*, conv2.conv.weight,
 * conv2.bn0.*, conv2.fc1.{weight,bias}, conv2.bn1.*, conv2.fc2.{weight,bias}, conv3.weight, bn3.*, [downsample.1.weight, downsample.2.*
 * when I == 0]; fc_ori / fc_shape / fc_exp / fc_tex {weight, bias}.  fc_tex is KEPT in flat, so a checkpoint flattens as it is:
 * 25 707 814 floats; the module never calls it and it is not packed.  BatchNorm is folded on the host in fp32 (eps 1e-5).
 * After loading, syn_backbone_forward[_u8] run this network, every product exact fp32 (fp32-input MFMA; means, gate, softmax and pools in
 * fp32 VALU in a fixed order): syn_numerics_report has nothing to prove, syn_backbone_range_status / _calibrate return 0.  param = the
 * module's 62 outputs (ori 12 | shape 40 | exp 10), pool = the 2048 channel means: not 1280 wide, so syn_refine_landmarks refuses this arch.
 * SYNERGY_HIP_FUSION / syn_set_schedule(h, .): 0 = per-layer (95 launches: the split-attention sum, its 3x3 / 2 average and the
 * downsample's 2x2 / 2 average are stored, one launch each); 1 = fused (74 launches: conv3, and the downsample convolution of layer2.0 /
 * 3.0, build those operands once per workgroup in LDS; they never reach HBM); 2 (default) = as 1.  The schedules are bit-identical.
 * syn_resnest50_flops_per_face = 2 x 1 637 330 432 MAC: every product of the module's forward (Conv2d and Linear; fc_tex never runs). */
size_t syn_resnest50_flat_count(void);
double syn_resnest50_flops_per_face(void);
int syn_load_backbone_resnest50(syn_handle *h, const float *flat, size_t n_floats);

/* The BasicBlock ResNets (reference backbone_nets/resnet_backbone.py:50-87, 282-301; `--arch resnet18` / `--arch resnet34` of
 * main_train.py).  Backbone ids 10 and 11; the id table continues:
 *   9: never assigned | 10 resnet18 | 11 resnet34
 * `flat` = the module's state_dict() order without num_batches_tracked (synergynet_amd.synergy3DMM.resnet_basic_keys): conv1.weight, bn1.*,
 * then per BasicBlock layerL.I: conv1.weight, bn1.*, conv2.weight, bn2.*, [downsample.0.weight, downsample.1.* on layer2.0 / 3.0 / 4.0];
 * fc_tex / fc_ori / fc_shape / fc_exp {weight, bias}.  fc_tex is KEPT in flat, so a checkpoint flattens as it is: 11 238 438 floats
 * (resnet18), 21 354 022 (resnet34); it is not packed.  BatchNorm is folded on the host in fp32 (eps 1e-5).
 * After loading, syn_backbone_forward[_u8] run this network, every product exact fp32 (fp32-input MFMA): syn_numerics_report has nothing
 * to prove, syn_backbone_range_status / _calibrate return 0.  param = the first 62 of the module's 102 outputs (ori 12 | shape 40 |
 * exp 10; fc_tex does not run), pool = the 512 channel means: not 1280 wide, so syn_refine_landmarks refuses these archs.
 * SYNERGY_HIP_FUSION / syn_set_schedule(h, .): 0 = per-layer (22 / 38 launches: every 3x3 convolution reads its taps from global memory,
 * the 1x1 stride-2 downsample of layer2.0 / 3.0 / 4.0 is a launch of its own); 1 = LDS-tiled (19 / 35 launches: a workgroup stages a band
 * of input rows with its halo, or whole faces of the 8^2 / 4^2 maps, once in LDS, at most 80 KiB, and conv1 of those three blocks also
 * produces the downsample from its centre tap); 2 (default) = as 1.  The schedules are bit-identical.
 * syn_resnet_basic_flops_per_face = 2 x the MACs the forward runs (Conv2d and the three heads): 2 x 553 011 200 (resnet18),
 * 2 x 1 129 564 160 (resnet34).  An arch other than 10 / 11: the counts return 0, the loader SYN_ERR_INVALID. */
size_t syn_resnet_basic_flat_count(int arch);
double syn_resnet_basic_flops_per_face(int arch);
int syn_load_backbone_resnet_basic(syn_handle *h, int arch, const float *flat, size_t n_floats);

/* ParamsPack (utils/params.py:10-35) + the register_buffer block (synergy3DMM.py:95-105).
 * HOST arrays: w_shp [3*n_vert,40], w_exp [3*n_vert,10], u [3*n_vert] (= u_shp+u_exp),
 * param_mean/param_std [>=62] (first 62 used), keypoints [3*n_lmk] flat indices into the
 * 3*n_vert axis ordered [3k,3k+1,3k+2] (utils/io.py:78-81). */
int syn_load_basis(syn_handle *h, const float *w_shp, const float *w_exp, const float *u,
                   const float *param_mean, const float *param_std,
                   const int64_t *keypoints, int n_lmk, int n_vert);

/* Multi-GPU: rank 0 loads from host arrays, exports its packed constants into a caller
 * device buffer, the caller broadcasts that buffer (RCCL, e.g. torch.distributed.broadcast)
 * and every other rank imports it.  No cross-GPU traffic after that. */
size_t syn_constants_bytes(syn_handle *h);
int syn_export_constants(syn_handle *h, void *dev_dst, size_t bytes, void *stream);
int syn_import_constants(syn_handle *h, const void *dev_src, size_t bytes, void *stream);
/* The same hand-off in ONE call for a caller that holds an RCCL communicator instead of torch.distributed (what replaces the
 * reference's nn.DataParallel replication, benchmark.py:112 / main_train.py:176): collective over `nccl_comm` (an ncclComm_t; every
 * rank calls it with its own handle, on the device the communicator was created for) -- rank `root` exports, ncclBroadcast ships the
 * size and then the blob, every other rank imports; returns after the stream has drained.  The library does not link RCCL: it
 * calls the instance the process already holds (the caller's, or torch's librccl.so.1), so the communicator and the code that
 * uses it always belong together (a process that holds more than one RCCL names the owner of the communicator with the environment
 * variable SYNERGY_HIP_RCCL_LIB = path of that librccl).  SYN_ERR_INVALID for a NULL communicator, SYN_ERR_NOT_LOADED when the process
 * holds no RCCL.
 * A COLLECTIVE THAT FAILS, FAILS ON EVERY RANK (csrc/bcast_protocol.h): a root handle without constants, or one that cannot stage its
 * blob, reports that inside the first broadcast (size word 0 + its code) and EVERY rank returns that code (SYN_ERR_NOT_LOADED /
 * SYN_ERR_HIP); a rank that cannot stage or import the blob reports it in an ncclAllReduce(max) of the status and every rank returns
 * it -- no rank is left waiting in a collective another rank never enters, and the communicator stays usable.  (The one local exit:
 * a rank that cannot allocate the 256-byte word buffer has no device memory to join a collective with.) */
int syn_bcast_constants(syn_handle *h, void *nccl_comm, int root, void *stream);
/* The 256-byte header syn_export_constants would write for this handle NOW (what it holds: arch, backbone / basis present, vertex and
 * landmark counts, total bytes), into HOST memory, no device call -- how a host mirror learns what a syn_bcast_constants import gave it. */
int syn_describe_constants(syn_handle *h, void *host_header, size_t bytes);

/* Device-free twins of the hand-off: neither makes a HIP call, so a loader process (or a test) without a GPU can produce and
 * vet the blob.  syn_pack_constants_host writes, from HOST arrays (same meaning as syn_load_backbone / _resnet50 / syn_load_basis;
 * backbone_flat or the whole basis group may be NULL), exactly the bytes syn_export_constants produces after the same loads;
 * arch 0 = mobilenet_v2, 1 = resnet50, 2 / 3 / 4 = mobilenet_1 / _05 / _2, 6 = ghostnet, 8 = resnest50, 10 / 11 = resnet18 / resnet34 (5, 7 and 9 were never assigned and are refused).  syn_check_constants_host applies syn_import_constants' acceptance checks (magic, version,
 * sizes vs this library's network tables, payload within the buffer) to a host copy of a blob. */
size_t syn_pack_constants_host_bytes(int arch, int have_backbone, int n_vert, int n_lmk);
int syn_pack_constants_host(int arch, const float *backbone_flat, size_t n_floats, const float *w_shp, const float *w_exp,
                            const float *u, const float *param_mean, const float *param_std, const int64_t *keypoints,
                            int n_lmk, int n_vert, void *host_dst, size_t bytes);
int syn_check_constants_host(const void *host_blob, size_t bytes);

/* ---- compute ------------------------------------------------------------------------ */

/* Bytes of activation workspace the library keeps for a batch of B faces. */
size_t syn_workspace_bytes(syn_handle *h, int B);

/* forward_test (synergy3DMM.py:151-154 -> mobilenetv2_backbone.py:173-189).
 * img   [B,3,120,120] fp32 NCHW, already (x-127.5)/128 (synergy3DMM.py:189-192)
 * param [B,62] (ori 0:12, shape 12:52, exp 52:62);  pool [B,1280] or NULL. */
int syn_backbone_forward(syn_handle *h, const float *img, int B, float *param, float *pool,
                         void *stream);

/* Same, from uint8 crops [B,120,120,3] (HWC, BGR as cv2 delivers them); the
 * (x-127.5)/128 normalisation and the HWC->CHW permute (synergy3DMM.py:189-192) are fused
 * into the first convolution. */
int syn_backbone_forward_u8(syn_handle *h, const uint8_t *img_hwc, int B, float *param,
                            float *pool, void *stream);

/* Pre-processing of get_all_outputs (synergy3DMM.py:187-188): crop_img (utils/inference.py:95-125, zero padding outside
 * the frame) + cv2.resize(..., (120,120), INTER_LANCZOS4) for B detections of ONE frame, on device.
 * frame [H,W,3] uint8 HWC; box [B,4] = int(round()) of the enlarged square box (sx,sy,ex,ey);
 * xofs/yofs [B,120] = first of the 8 source taps in crop coordinates, xcoef/ycoef [B,120,8] = OpenCV's 11-bit fixed
 * point Lanczos-4 weights (the host computes these tables: synergynet_amd/inference.py lanczos4_tables);
 * out [B,120,120,3] uint8, the input of syn_backbone_forward_u8.  All pointers are device pointers. */
int syn_crop_resize(syn_handle *h, const uint8_t *frame, int H, int W, const int *box, const int *xofs,
                    const int16_t *xcoef, const int *yofs, const int16_t *ycoef, uint8_t *out, int B, void *stream);

/* The same for the faces of SEVERAL frames in ONE launch (the reference loops over faces inside get_all_outputs, synergy3DMM.py:176-191,
 * and over images outside it; a caller with a list of frames -- synergynet_amd get_all_outputs_batch -- stages all of them in one device
 * block): frames = base of that block, frame_off [n_frames] byte offset of each frame in it, frame_dim [n_frames][2] = H, W of each,
 * face_frame [B] = frame index of face b; box / tables / out per face as above.  Same arithmetic per face: same bytes. */
int syn_crop_resize_frames(syn_handle *h, const uint8_t *frames, const long long *frame_off, const int *frame_dim,
                           const int *face_frame, const int *box, const int *xofs, const int16_t *xcoef, const int *yofs,
                           const int16_t *ycoef, uint8_t *out, int B, void *stream);

/* The tables above computed on the device, so that detections never visit the host between the detector and the crop
 * (synergynet_amd get_all_outputs_frames).  All pointers are device pointers; n == 0 / N == 0 is SYN_OK without a launch; NULL
 * pointers and negative sizes are SYN_ERR_INVALID with nothing enqueued.
 *
 * syn_lanczos4_tables: the tap tables of synergynet_amd/inference.py lanczos4_tables(side, 120) for n crop sides: ofs [n,120],
 * coef [n,120,8], the same integers as the host function for every side (same rounding points: source position in double rounded
 * to float32, eight weights in double rounded to float32, float32 sum tap 0 first, 11-bit fixed point).  The sides are the
 * caller's own numbers, so this call reads them back first (it synchronises `stream`) and refuses a side < 1. */
int syn_lanczos4_tables(syn_handle *h, const int *sides, int n, int *ofs, int16_t *coef, void *stream);

/* Everything syn_crop_resize_frames and syn_landmarks_pose / syn_reconstruct need per face, from n FLOAT32 detections
 * dets [n,5] (x1, y1, x2, y2, score) as the detector leaves them: roi [n,5] = the enlarged square box of get_all_outputs
 * (synergy3DMM.py:178-185: centre +- floor(height * 1.2 / 2)) and the score, in float32 arithmetic like numpy's on float32
 * detections; box [n,4] = rint(roi[0:4]) (ties to even, utils/inference.py:98); xofs / xcoef and yofs / ycoef = the tables of
 * syn_lanczos4_tables for the box's width and height.  status [n]: non-zero exactly where the host path raises 'degenerate
 * detection box' (a non-finite or > 2^30 rounded coordinate, width or height <= 0 or beyond int32); such a face keeps its float roi,
 * gets box (0,0,1,1) and the taps of side 1 -- the crop kernel runs over it harmlessly -- and no other face is affected.  Only
 * enqueues on `stream`; the caller reads status with its results. */
int syn_face_tables(syn_handle *h, const float *dets, int n, float *roi, int *box, int *xofs, int16_t *xcoef, int *yofs,
                    int16_t *ycoef, int *status, void *stream);

/* The vis_thres filter of FaceBoxes.__call__ (FaceBoxes.py:131-141) over the padded rows of syn_detect_batch: dets [N,K,5],
 * counts [N] rows valid per frame (clamped to 0..K; rows past the count are never read).  Output frame i reads input row
 * order[i] (order NULL: i; an index outside 0..N-1 is a frame without faces) -- the way from size groups back to input order.
 * rows [N*K,5]: the rows with score > thres (strict; NaN is not greater), frame after frame, each frame's in their order;
 * face_frame [N*K]: the output frame of each; frame_faces [N+1]: faces per output frame, then their total.  Entries of rows /
 * face_frame past the total are left as they were.  One workgroup; only enqueues on `stream`. */
int syn_compact_detections(syn_handle *h, const float *dets, const int *counts, const int *order, int N, int K, float thres,
                           float *rows, int *face_frame, int *frame_faces, void *stream);

/* reconstruct_vertex_62 (synergy3DMM.py:116-149) fused with the ROI affine of
 * _predict_vertices (utils/inference.py:127-138).
 * param [B,param_len] whitened; param_len must be 62 (else SYN_ERR_PARAM_LEN).
 * dense: 0 -> out [B,3,n_lmk], 1 -> out [B,3,n_vert].
 * transform: y -> 121 - y (synergy3DMM.py:139,147).
 * roi [B,5] (sx,sy,ex,ey,score) or NULL for no ROI affine (the batched torch method). */
int syn_reconstruct(syn_handle *h, const float *param, int B, int param_len, int dense,
                    int transform, const float *roi, float *out, void *stream);

/* Same contraction into a PITCHED output: the rows of out (one per face and coordinate) start row_pitch floats apart,
 * row_pitch >= n (n = n_vert or n_lmk); syn_reconstruct is row_pitch = n.
 * pad_writable != 0: the caller owns columns [n, row_pitch) of every row too (out is B*3*row_pitch floats long, the last
 * row included) and allows them to be overwritten with unspecified finite values; 0: they are left untouched.
 * Why: the reference's result is a [B,3,53215] tensor (synergy3DMM.py:131-147) whose rows are 212860 bytes, so packed rows
 * are only 4-byte aligned and every store run shares HBM lines with its neighbours (measured 3.3 TB/s of writes).  With
 * row_pitch = n rounded up to a multiple of 128 floats (53248), a 128-byte aligned out and writable pad columns every run
 * is whole lines (5.2 TB/s) and the kernel takes its branch-free store path.  A torch view `storage[:, :, :n]` of a
 * [B,3,row_pitch] allocation has the reference's shape and values. */
int syn_reconstruct_pitched(syn_handle *h, const float *param, int B, int param_len, int dense,
                            int transform, const float *roi, float *out, int row_pitch, int pad_writable, void *stream);

/* ---- mesh consumers: what the reference's demo does with the meshes (utils/render.py:31-50) ----
 * syn_load_triangles: the mesh topology (param_pack `tri`, 0-based, [ntri,3] int32 host pointer), once per handle;
 * replaces the `triangles` argument of Sim3DR.get_normal / rasterize (Sim3DR/Sim3DR.py:8,14). */
int syn_load_triangles(syn_handle *h, const int32_t *tri, int ntri, int nver);

/* Sim3DR.get_normal (Sim3DR/Sim3DR.py:8-11 -> lib/rasterize_kernel.cpp:158-215) and, when light != NULL, the vertex
 * colours of RenderPipeline.__call__ (Sim3DR/lighting.py:37-64) for F meshes in one launch chain.
 * vertices: device, planar = 1 -> [F,3,nver] (what syn_reconstruct writes), 0 -> [F,nver,3] (the reference's layout),
 *           planar = p >= nver (p > 1) -> [F,3,p][:, :, :nver], rows p floats apart: the pitched tensor syn_reconstruct_pitched
 *           writes, consumed in place (no packed copy anywhere between reconstruction and rendering);
 * normal, light: device [F,nver,3] (light may be NULL);
 * cfg16: HOST pointer to 16 floats: intensity_ambient, color_ambient[3], intensity_directional, color_directional[3],
 *        intensity_specular, specular_exp, light_pos[3], view_pos[3] (lighting.py:24-32). */
int syn_mesh_shade(syn_handle *h, const float *vertices, int F, int planar, const float *cfg16, float *normal,
                   float *light, void *stream);

/* Sim3DR.rasterize (Sim3DR/Sim3DR.py:14-29 -> lib/rasterize_kernel.cpp:219-287, alpha = 1 as the binding defaults):
 * draws F meshes, in order, into image [H,W,channels] uint8 (device, in place), each with a fresh z-buffer, i.e. the
 * result of calling the reference once per mesh on the same background.  colors: device [F,nver,channels] float32 in [0,1].
 * F <= 254, channels <= 4.  reverse: flip y on write (rasterize_kernel.cpp:270). */
int syn_rasterize(syn_handle *h, const float *vertices, const float *colors, int F, int planar, int channels,
                  uint8_t *image, int H, int W, int reverse, void *stream);

/* cv2.addWeighted(a, alpha, b, beta, 0) for uint8 arrays of n bytes (utils/render.py:45), device pointers. */
int syn_add_weighted(syn_handle *h, const uint8_t *a, float alpha, const uint8_t *b, float beta, uint8_t *out,
                     size_t n, void *stream);

/* ---- textured meshes: what the reference's texture demos do with a mesh (uv_texture_realFaces.py:45-51,96-116, artistic.py:44-49,111-117) ----
 * syn_load_uv_map: the UV assets, once per handle (HOST int32 arrays).
 *   coord_u, coord_v [nver]: pixel row / column of every vertex in the UV texture image, (uv[:,1]*255.0).astype(int32) and
 *     (uv[:,0]*255.0).astype(int32) of 3dmm_data/BFM_UV.npy -- the caller evaluates them in the asset's own dtype (:48-49);
 *   keep_ind [n_keep]: the kept vertex subset (keptInd.npy), indices into the nver vertices;
 *   tri_kept [ntri_kept,3]: 0-based topology of the KEPT vertex list (deletedTri.npy is 1-based [3,ntri]: pass its transpose - 1).
 * The kept topology goes into a second topology slot with its own adjacency, next to the one syn_load_triangles holds, so a
 * caller that alternates full-mesh and textured renders re-uploads neither.  Index ranges are validated like syn_load_triangles. */
int syn_load_uv_map(syn_handle *h, const int32_t *coord_u, const int32_t *coord_v, int nver, const int32_t *keep_ind, int n_keep,
                    const int32_t *tri_kept, int ntri_kept);

/* Which topology syn_mesh_shade, syn_mesh_shade_textured and syn_rasterize work on from now on: 0 = syn_load_triangles' (the
 * default, and what every syn_load_triangles call selects), 1 = the kept topology of syn_load_uv_map (vertex count n_keep).
 * SYN_ERR_NOT_LOADED when that slot is empty. */
int syn_select_topology(syn_handle *h, int slot);

/* np.flip(img, axis=0)[coord_u, coord_v, :] (uv_texture_realFaces.py:109-110) for T texture images in one launch.
 * uv_tex: device uint8 [T,tex_h,tex_w,channels] (channels <= 4); kept != 0: one colour per kept vertex (n = n_keep, vertex keep_ind[k]),
 * else per vertex (n = nver); out: device float32 [T,n,channels], out[t,k,:] = uv_tex[t, tex_h-1-coord_u[v], coord_v[v], :] as
 * 0..255 (normalize = 0, what the coloured OBJ takes, :113) or divided by 255.0f (one IEEE division, :115).
 * SYN_ERR_INVALID when the texture is smaller than the table needs. */
int syn_uv_colors(syn_handle *h, const uint8_t *uv_tex, int T, int tex_h, int tex_w, int channels, int kept, int normalize, float *out,
                  void *stream);

/* vertices[:, keep_ind] (uv_texture_realFaces.py:98) for F meshes: vertices device [F,3,nver] (planar = 1) or the pitched
 * [F,3,p][:, :, :nver] (planar = p >= nver) read in place; out device [F,3,n_keep] packed. */
int syn_gather_vertices(syn_handle *h, const float *vertices, int F, int planar, float *out, void *stream);

/* syn_mesh_shade with `texture *= light` (Sim3DR/lighting.py:68-70) in the lighting kernel's epilogue, on the selected topology.
 * vertices, planar, cfg16, normal as syn_mesh_shade; light: device [F,nver,3] or NULL; colors: device [F,nver,3], what syn_rasterize draws.
 * shared = 0: tex device [F,nver,3], colors[f] = tex[f] * light[f] (colors may be tex itself).
 * shared = 1: tex device [nver,3], ONE array multiplied in place face after face as the reference does when utils/render.py:39-42
 *   hands the same array to every call: colors[f] = ((tex * light[0]) * light[1]) ... * light[f] in float32, left to right, and tex
 *   holds the last product afterwards. */
int syn_mesh_shade_textured(syn_handle *h, const float *vertices, int F, int planar, const float *cfg16, float *normal, float *light,
                            float *tex, int shared, float *colors, void *stream);

/* ---- visibility buffers: Sim3DR.rasterize_triangles and the way from a photograph to a UV texture image ----
 * All four work on the topology syn_select_topology selected, take `planar` as syn_mesh_shade does, enqueue on `stream` and
 * synchronise nothing.
 *
 * syn_rasterize_triangles: Sim3DR.rasterize_triangles (Sim3DR/lib/rasterize.pyx:74-86 -> rasterize_kernel.cpp:290-348) for F meshes,
 * each into its OWN planes: per pixel the triangle that wins the depth test (the deepest; the earliest index among equal depths,
 * +0 and -0 being equal), its depth and its barycentric weights (order 1-u-v, v, u).
 * depth_buffer [F,H,W] float32, triangle_buffer [F,H,W] int32, barycentric_weight [F,H,W,3] float32: device, IN-OUT.  The caller
 * initialises them (the usual values are -1e8, -1 and 0), exactly as the reference's binding leaves that to its caller: a
 * triangle competes for a pixel only where its depth is greater than the caller's depth_buffer (NaN never is), and pixels no
 * triangle wins keep the caller's values in all three.  Any F (no face field in the key; the key planes come from the render
 * scratch, which grows on demand); F*H*W >= 2^31 is SYN_ERR_INVALID. */
int syn_rasterize_triangles(syn_handle *h, const float *vertices, int F, int planar, float *depth_buffer, int32_t *triangle_buffer,
                            float *barycentric_weight, int H, int W, void *stream);

/* Per-vertex visibility, the rule of the 3DDFA lineage: a vertex is visible when it is a corner of a triangle that won at least
 * one pixel.  triangle_buffer: device [F,H,W] int32 as syn_rasterize_triangles leaves it (values outside [0, ntri) mark nothing);
 * visible: device [F,nver] uint8, zeroed by the call, 1 where visible. */
int syn_vertex_visibility(syn_handle *h, const int32_t *triangle_buffer, int F, int H, int W, uint8_t *visible, void *stream);

/* One colour per vertex from a frame: bilinear sample of image (device uint8 [H,W,channels], channels <= 4) at the vertex' (x, y),
 * in the operation order of the reference's bilinear code (rasterize_kernel.cpp:428-447): x clamped to [0,W-1], y to [0,H-1],
 * xd = x - floor(x), yd likewise, ul*(1-xd)*(1-yd) + ur*xd*(1-yd) + dl*(1-xd)*yd + dr*xd*yd, left to right in float32.
 * out: device float32 [F,nver,channels], 0..255 (normalize = 0) or divided by 255.0f (one IEEE division).  A vertex whose x or y is
 * not finite gets colour 0. */
int syn_sample_vertex_colors(syn_handle *h, const float *vertices, int F, int planar, const uint8_t *image, int H, int W, int channels,
                             int normalize, float *out, void *stream);

/* The inverse of syn_uv_colors over ALL vertices of the UV table (needs syn_load_uv_map, SYN_ERR_NOT_LOADED otherwise): for every face
 * tex[f, tex_h-1-coord_u[v], coord_v[v], :] = uint8(clip(rint(colors[f,v,:]), 0, 255)) and mask[f, ...] = 255 for every vertex v with
 * visible[f,v] != 0 (visible == NULL: every vertex).  Where several vertices share a texel the highest vertex index wins (numpy's
 * in-order assignment); texels no vertex lands on are 0 in both.  Every texel of tex and mask is written.
 * colors: device float32 [F,nver,channels] in 0..255; visible: device uint8 [F,nver] or NULL; tex: device uint8 [F,tex_h,tex_w,channels];
 * mask: device uint8 [F,tex_h,tex_w].  SYN_ERR_INVALID when the texture is smaller than the table needs. */
int syn_uv_scatter(syn_handle *h, const float *colors, const uint8_t *visible, int F, int channels, uint8_t *tex, uint8_t *mask, int tex_h,
                   int tex_w, void *stream);

/* Fills the texels no vertex wrote: deterministic push-pull (pyramid) completion of uint8 UV textures, integer arithmetic only, so the
 * result is defined byte for byte (tests/texture_fill_cases.py states it in numpy).
 *   level 0  w = (mask != 0), c = tex * w per channel.  merge != 0: the T views collapse into ONE texture, w = sum_t (mask_t != 0),
 *            c = sum_t tex_t * (mask_t != 0).
 *   push     level l+1 is ceil(H_l/2) x ceil(W_l/2); w and c are the plain sums over the up-to-four children that exist.
 *   own      where w > 0: floor((2c + w) / (2w)) (round half up).
 *   pull     from the 1x1 level down: V = own where w > 0, elsewhere (9 V[py,px] + 3 V[py,nx] + 3 V[ny,px] + V[ny,nx] + 8) >> 4 on the
 *            level above, py = y >> 1, ny = clamp(py + (y odd ? +1 : -1), 0, H_{l+1} - 1), px / nx likewise.  tex_out = V_0.
 * Valid texels keep their value (merged: the rounded mean of the views that saw them); a texture without a valid texel comes out 0.
 * tex_in: device uint8 [T,tex_h,tex_w,channels]; mask: device uint8 [T,tex_h,tex_w], nonzero = valid, not modified; tex_out: device
 * uint8 [T,tex_h,tex_w,channels], or [1,tex_h,tex_w,channels] with merge.  Three launches on `stream` whatever T and the size, nothing
 * is synchronised; the pyramid lives in the render scratch.  SYN_ERR_INVALID (nothing enqueued): a NULL pointer, T < 1, channels
 * outside 1..4, tex_h or tex_w outside 1..4096, tex_out overlapping tex_in or mask, merge with T*tex_h*tex_w > 2^24 (the sums would
 * not fit 32 bits). */
int syn_texture_fill(syn_handle *h, const uint8_t *tex_in, const uint8_t *mask, int T, int tex_h, int tex_w, int channels, int merge,
                     uint8_t *tex_out, void *stream);

/* ---- per-pixel texture mapping: the reference's _render_texture_core (Sim3DR/lib/rasterize_kernel.cpp:353-458, binding commented
 * out in rasterize.pyx:24-31,104-123), a z-buffer walk that samples a texture IMAGE per pixel instead of interpolating vertex colours ----
 * syn_load_tex_coords: the texture coordinates of the currently selected topology slot (HOST arrays), stored on the device per slot
 * until that slot's topology is replaced.  tex_coords [tex_nver,3] float32: x = texture column, y = texture row, in texels (the third
 * column is not read; row stride 3 as in the reference); tex_triangles [ntri,3] int32, ntri = the slot's triangle count, or NULL for
 * the slot's own mesh triangles.  Validated like syn_load_triangles: every tex_triangles index in [0, tex_nver), and every index of
 * the slot's MESH triangles < tex_nver (see quirk 2).  SYN_ERR_NOT_LOADED when the slot is empty. */
int syn_load_tex_coords(syn_handle *h, const float *tex_coords, int tex_nver, const int32_t *tex_triangles);

/* syn_render_texture: F meshes of the selected topology drawn into image / depth_buffer (device, IN-OUT) with a per-pixel texture
 * lookup.  All arithmetic is float32 in the reference's operation order, without FMA contraction; with a float32 texture and image the
 * result is bit-identical to the reference's compiled function.
 *   candidates  triangle i competes for pixel (x, y) when the pixel lies in max(ceil(min),0) .. min(floor(max),W-1) of its corners
 *               (likewise in y: the box of _rasterize_triangles) and  x < 2 || x > W-3 || y < 2 || y > H-3 || is_point_in_tri.
 *               Quirk 1, kept: on the two-pixel frame border the inside test is bypassed (:418) and the weights are extrapolated,
 *               (1,0,0) for a zero-area triangle.
 *   depth test  p_depth = w0*d0 + w1*d1 + w2*d2, weights (1-u-v, v, u); a candidate competes only where p_depth > the caller's
 *               depth_buffer (NaN never does); the greatest depth wins, the earliest index among equals, +0 == -0; the stored depth
 *               is the winner's own value (a zero keeps its sign).
 *   coordinate  tex_p = tex_p0*w0 + tex_p1*w1 + tex_p2*w2, left to right.  Quirk 2, kept: x is read through tex_triangles, y through
 *               the MESH triangle's indices (:393-398).  Quirk 3, kept: tex_coords has row stride 3.  With tex_triangles == the mesh
 *               triangles (NULL above) quirk 2 vanishes.
 *   clamp       x = x > tex_w-1 ? tex_w-1 : x;  x = x >= 0 ? x : 0  (y likewise): the reference's max(min()) for every finite value.
 *               DEFINED here where the reference is not: a NaN coordinate samples coordinate 0 (the reference converts NaN to int
 *               and reads out of range).
 *   sample      mapping_type 0: texture[int(round(y)), int(round(x)), k], round half away from zero; 1: xd = x - floor(x), yd
 *               likewise, ul*(1-xd)*(1-yd) + ur*xd*(1-yd) + dl*(1-xd)*yd + dr*xd*yd left to right over floor / ceil neighbours.
 *               Channels k < c of the image come from channels k of the tex_c-channel texture.  Pixels nobody wins keep the caller's
 *               image and depth.
 * vertices, planar: as syn_mesh_shade.  texture: device [T,tex_h,tex_w,tex_c], float32 (tex_u8 = 0) or uint8 (tex_u8 = 1, read as
 * (float)byte: identical to converting first), T = 1 (one for all faces) or F.  image: float32 (image_u8 = 0) or uint8 (image_u8 = 1:
 * winners stored as uint8(clip(rint(v), 0, 255)), the convention of syn_uv_scatter; goes straight into syn_add_weighted).
 * shared = 0: image [F,H,W,c], depth_buffer [F,H,W], every mesh its own planes, like syn_rasterize_triangles.
 * shared = 1: image [H,W,c], depth_buffer [H,W]: the result of calling the reference once per mesh, in order, on the SAME image and
 *   depth buffer -- all faces compete in one z-buffer, the earliest (face, triangle) wins among equal depths.
 * Two launches on `stream`, nothing is synchronised; the key planes come from the render scratch, which grows on demand.
 * SYN_ERR_NOT_LOADED: no topology, or no texture coordinates for the selected slot.  SYN_ERR_INVALID, nothing enqueued: a NULL pointer,
 * c outside 1..4, c > tex_c, tex_c > 4, T not in {1, F}, mapping_type not in {0, 1}, F*ntri >= 2^32, F*H*W >= 2^31, F > 65535, a
 * texture side above 2^24 or T*tex_h*tex_w >= 2^31, a bad planar. */
int syn_render_texture(syn_handle *h, const float *vertices, int F, int planar, const void *texture, int tex_u8, int T, int tex_h, int tex_w,
                       int tex_c, int mapping_type, void *image, int image_u8, float *depth_buffer, int H, int W, int c, int shared,
                       void *stream);

/* ---- FaceBoxes face detector: the boxes get_all_outputs crops (synergy3DMM.py:169-171) ----
 * syn_detector_flat_count / syn_load_detector: FaceBoxesNet's state_dict (FaceBoxes/models/faceboxes.py:64-114) flattened in
 * forward order -- conv1, conv2, inception{1,2,3}.{branch1x1, branch1x1_2, branch3x3_reduce, branch3x3, branch3x3_reduce_2,
 * branch3x3_2, branch3x3_3}, conv3_1, conv3_2, conv4_1, conv4_2: weight [cout,cin,k,k] | bn weight | bias | running_mean |
 * running_var;  then loc.i, conf.i (i = 0..2): weight | bias.  Host pointer. */
size_t syn_detector_flat_count(void);
int syn_load_detector(syn_handle *h, const float *flat, size_t count);
/* number of priors for a network input of Hs x Ws pixels (FaceBoxes/utils/prior_box.py:20) */
int syn_detector_prior_count(int Hs, int Ws);
/* FaceBoxes.__call__ (FaceBoxes/FaceBoxes.py:60-127) on one uint8 BGR frame [H,W,3] (device): optional bilinear down-scaling
 * to Hs x Ws = int(scale*H) x int(scale*W), which the CALLER evaluates in double precision exactly like :63-75 (a float32
 * product lands one pixel off on ~8 % of frame sizes); Hs = H, Ws = W, scale = 1 for no scaling.  Then mean subtraction,
 * network, priors, decoding (boxes * (Ws,Hs,Ws,Hs) / scale, :101-104), score > conf_thr, top_k by score (any number of
 * candidates; top_k <= 8192), NMS (cpu_nms.pyx semantics, IoU >= nms_thr suppresses), first keep_top_k rows.
 * dets: device [keep_top_k,5] (x1, y1, x2, y2, score) in original-frame pixels, score-descending; n_dets: HOST int, rows
 * valid (the call synchronises `stream`).  The vis_thres filter (:133-140) is the caller's.  It is the N = 1 case of
 * syn_detect_batch's launches plus the download of the count. */
int syn_detect(syn_handle *h, const uint8_t *frame, int H, int W, int Hs, int Ws, float scale, float conf_thr, float nms_thr,
               int top_k, int keep_top_k, float *dets, int *n_dets, void *stream);
/* The same detector on N frames of ONE size in the same launches (a frame index on every kernel; the weights are shared): frames
 * device [N,H,W,3] uint8 BGR, contiguous; H, W, Hs, Ws, scale and the thresholds as above, for all frames.  Per frame the rows are
 * bit for bit those of the single-frame call on that frame, whatever N and the neighbours are.  dets: device [N,keep_top_k,5];
 * n_dets: DEVICE int [N], rows valid per frame.  The call only enqueues on `stream` (the candidate counters are reset there by
 * the call itself) and synchronises nothing; the one exception is a call that needs more scratch than any before it on this
 * handle, which waits for the device before the workspace is reallocated.  Calls on one handle share that workspace: enqueue
 * them on one stream (or order the streams).  Refused with nothing enqueued: NULL pointers, N outside
 * 1..SYN_DETECT_BATCH_MAX_FRAMES, the argument ranges the single-frame call refuses (top_k > 8192 included), weights not loaded, a
 * batch whose scratch would exceed SYN_DETECT_BATCH_MAX_SCRATCH_BYTES (about 8.2 floats, 33 bytes, per pixel of the
 * Hs x Ws network input: 25 MB per 720x1080 frame, 0.41 GB for 16 of them, about 40 fit; split larger batches into several calls). */
#define SYN_DETECT_BATCH_MAX_FRAMES 1024
#define SYN_DETECT_BATCH_MAX_SCRATCH_BYTES ((size_t)1 << 30)
int syn_detect_batch(syn_handle *h, const uint8_t *frames, int N, int H, int W, int Hs, int Ws, float scale, float conf_thr,
                     float nms_thr, int top_k, int keep_top_k, float *dets, int *n_dets, void *stream);

/* calc_nme (benchmark_aflw2000.py:107-139): fit [N,2,68] fitted landmarks in 120x120 crop coordinates, gt [N,3,68] ground truth
 * in image coordinates, roi [N,4] crop boxes (sx, sy, ex, ey) -> nme [N] float32.  All device pointers. */
int syn_nme(syn_handle *h, const float *fit, const float *gt, const float *roi, float *nme, int N, void *stream);

/* predict_pose (utils/inference.py:146-157 -> parse_pose :86-92 -> P2sRt :33-43 ->
 * matrix2angle_corr :45-62).  angles [B,3] degrees (double, like the reference's python
 * floats), t3d [B,3] fp32 with the ROI affine on x,y; roi may be NULL. */
int syn_pose(syn_handle *h, const float *param, int B, const float *roi, double *angles,
             float *t3d, void *stream);

/* Landmarks AND pose of a batch in one launch: lmk [B,3,n_lmk] (packed rows) = syn_reconstruct(dense = 0, roi) and angles / t3d =
 * syn_pose(roi) -- what the reference's get_all_outputs computes per face besides the mesh (synergy3DMM.py:194-201: predict_sparseVert
 * + predict_pose; utils/inference.py:127-157).  The two calls above remain the boundary; this one exists because as separate calls
 * the three dependent launches (prologue, contraction, pose) are ~19 us of a 128-face landmarks-only step, one launch is ~6.  The
 * contraction runs as plain fp32 multiply-adds on the exact fp32 landmark basis (no fp16 pieces): equal to syn_reconstruct's landmarks
 * to fp32 rounding (~1e-6 of the largest coordinate); translation bit-identical to syn_pose, angles within 1e-4 degree of it.  SYN_ERR_PARAM_LEN for param_len != 62. */
int syn_landmarks_pose(syn_handle *h, const float *param, int B, int param_len, int transform, const float *roi /*nullable [B,5]*/,
                       float *lmk, double *angles /*[B,3] degrees*/, float *t3d /*[B,3]*/, void *stream);

/* predict_pose(..., ret_mat=True) (utils/inference.py:146-157): parse_pose's P = [R | t3d] "without scale" (:86-92),
 * pmat [B,3,4] fp32 row-major; R = normalised rows 0,1 of the de-whitened camera matrix and their cross product, column 3 =
 * the de-whitened translation WITHOUT the ROI affine (the reference concatenates P before predict_pose rescales t3d). */
int syn_pose_matrix(syn_handle *h, const float *param, int B, float *pmat, void *stream);

/* ---- synergy refinement: MLP_for (landmark residual) and MLP_rev (landmarks -> parameters) ----
 *
 * The two point-MLPs of the reference model (backbone_nets/pointnet_backbone.py; built at synergy3DMM.py:82-84 and used at
 * model_building.py:149-153):   Lr = Lc + 0.05 * MLP_for(Lc, pool, param[:,12:52], param[:,52:62]),   param_S2 = MLP_rev(Lr).
 * Every GEMM runs on the exact fp32 matrix instruction; a face's result does not depend on the batch it is in.
 *
 * FLAT layout (syn_synergy_flat_count floats): the tensors of MLP_for(68).state_dict() and then MLP_rev(68).state_dict() in
 * state_dict order without num_batches_tracked (checkpoint keys forwardDirection.* / reverseDirection.*), i.e. per MLP all convs
 * (weight [out,in,1] then bias) followed by all BatchNorms (weight, bias, running_mean, running_var).
 *
 * FOLDED layout (syn_synergy_folded_count floats, logical -- the device repack is private): per layer W [out][in] | scale [out] |
 * shift [out] with scale = gamma / sqrt(var + 1e-5) and shift = (bias - mean) * scale + beta, so y = relu(scale * (W x) + shift):
 *   MLP_for: conv1 [64][3], conv2 [64][64], conv3 [64][64], conv4 [128][64], conv5 [1024][128],
 *            conv6 split by input column: Wpoint [512][64] (point features) | Wface [512][2354] (global 1024 | pool 1280 | shape 40 |
 *            expr 10) | scale [512] | shift [512],  conv7 [256][512], conv8 [128][256], conv9 [3][128]
 *   MLP_rev: conv1 .. conv5 as above, then the three heads as ONE layer [62][1024] in the order ori 12 | shape 40 | expr 10. */
size_t syn_synergy_flat_count(void);
size_t syn_synergy_folded_count(void);
/* Device-free fold of a flat state into the folded layout (like syn_pack_constants_host).  SYN_ERR_INVALID on wrong counts. */
int syn_fold_synergy_host(const float *flat, size_t n, float *folded, size_t n_folded);

/* Folds `flat`, repacks it for the kernels and uploads it (6.4 MB); calling it again replaces the weights.  The weights are NOT part
 * of the constants blob (syn_export_constants): every rank loads them itself. */
int syn_load_synergy(syn_handle *h, const float *flat, size_t n);

/* Refined landmarks from whitened parameters and the backbone's 1280-d pooled feature.  Lc is reconstructed exactly as
 * syn_landmarks_pose does (crop space; transform = 1: with the y flip the MLP was trained on) and MLP_for runs on it with the
 * whitened shape / expression codes; lmk_refined = Lc + 0.05 * residual (the residual is relu'd by the reference: never negative).  With
 * roi both outputs receive the ROI affine x * sx + x0 / y * sy + y0 / z * (sx + sy) / 2 with sx = (ex - x0) / 120 (lmk_coarse then
 * equals syn_landmarks_pose(roi) bit for bit).  global_feat: MLP_for's max-pooled feature.  lmk_coarse and lmk_refined must not
 * overlap.  Scratch (33.8 KB per face, shared by the three entry points) is owned by the handle and grows lazily: calls on one handle
 * must be ordered on one stream, and the FIRST call at a new largest B frees and reallocates it behind a device-wide synchronisation
 * -- it stalls every stream once and must not happen inside a stream capture (run the largest batch once before capturing).
 * SYN_ERR_NOT_LOADED before syn_load_synergy / syn_load_basis; SYN_ERR_INVALID for B <= 0 or NULL pointers or overlapping outputs or
 * a handle whose backbone is resnet50 or a MobileNetV1 (their pooled features are not 1280-d: the refinement is unavailable there;
 * ghostnet's is 1280-d and is accepted). */
int syn_refine_landmarks(syn_handle *h, const float *param /*[B 62] whitened*/, const float *pool /*[B 1280]*/, int B, int transform,
                         const float *roi /*nullable [B 5]*/, float *lmk_coarse /*nullable [B 3 68]*/, float *lmk_refined /*[B 3 68]*/,
                         float *global_feat /*nullable [B 1024]*/, void *stream);

/* The same MLP on landmarks the caller supplies (crop space): no reconstruction and no ROI.  lmk_refined must not overlap lmk. */
int syn_refine_points(syn_handle *h, const float *lmk /*[B 3 68]*/, const float *pool, const float *param, int B, float *lmk_refined,
                      float *global_feat /*nullable*/, void *stream);

/* MLP_rev: landmarks [B,3,68] in crop space -> whitened parameters [B,62] (ori 12 | shape 40 | expr 10; relu'd like the reference). */
int syn_landmarks_to_param(syn_handle *h, const float *lmk /*[B 3 68]*/, int B, float *param /*[B 62]*/, void *stream);

/* ---- losses of the training graph's forward (model_building.py:141-157, loss_definition.py) ---- */

/* WingLoss of pred / target [B,3,n_points] -> one float.  d = |target - pred| per element; d < omega: omega log(1 + d / epsilon), else
 * d - C with C = omega - omega log(1 + omega / epsilon); the sum of the terms over the number of elements that took a branch.  As in the
 * reference d == omega is linear, a NaN d takes neither branch (neither summed nor counted; all NaN: 0 / 0 = NaN), d = inf gives inf.
 * Sums in fp64 in an order fixed by B * n_points alone, no floating-point atomics: the same bits on every call and every handle.
 * Scratch and ordering as syn_refine_landmarks (the handle's synergy scratch; calls on one handle on one stream).  Any backbone.
 * SYN_ERR_INVALID for NULL pointers, B <= 0, n_points < 1, omega or epsilon not positive; `loss` is then untouched. */
int syn_wing_loss(syn_handle *h, const float *pred, const float *target, int B, int n_points, float omega, float epsilon,
                  float *loss /*1 float*/, void *stream);

/* ParamLoss per face, input / target [B,62] -> loss [B].  mode 0 ('normal'): sqrt(mean((a[:12] - b[:12])^2) + mean((a[12:62] - b[12:62])^2));
 * mode 1 ('only_3dmm'): sqrt(mean((input[:50] - target[12:62])^2)) -- the slices are the reference's own.  A face's loss has the same
 * bits alone and at any position of any batch.  Any backbone, no scratch.  SYN_ERR_INVALID for NULL pointers, B <= 0, another mode. */
int syn_param_loss(syn_handle *h, const float *input /*[B 62]*/, const float *target /*[B 62]*/, int B, int mode /*0 normal | 1 only_3dmm*/,
                   float *loss /*[B]*/, void *stream);

/* SynergyNet.forward(input, target) behind the backbone: the landmarks of `param` and of `target` (as syn_landmarks_pose makes them: crop
 * space, transform = 1, no ROI), MLP_for on the predicted landmarks, MLP_rev on the refined ones, then ONE launch for the five weighted
 * losses -- all enqueued on `stream`, no host synchronisation.
 *   scalars[0] = loss_LMK_f0       = 0.05  WingLoss(landmarks(param), landmarks(target))
 *   scalars[1] = loss_LMK_pointNet = 0.05  WingLoss(refined landmarks, landmarks(target))
 *   per_face[0][b] = loss_Param_In   = 0.02  ParamLoss(param, target)
 *   per_face[1][b] = loss_Param_S2   = 0.02  ParamLoss(param_rev, target, only_3dmm)
 *   per_face[2][b] = loss_Param_S1S2 = 0.001 ParamLoss(param_rev, param, only_3dmm)
 * meter (nullable, 8 doubles on the device, zeroed by the caller before the first batch; one call at a time per meter):
 *   [i] += (batch mean of loss i) * B for the five losses in the order above, [5] += (sum of the five means) * B, [6] += B, [7] += 1
 *   -- AverageMeter.update(mean, B) of main_train.py:128-134; [i] / [6] is the running average.
 * Scratch (35.8 KB per face) and its caveat as syn_refine_landmarks.  SYN_ERR_NOT_LOADED before syn_load_synergy / syn_load_basis;
 * SYN_ERR_INVALID for B <= 0, NULL pointers or a backbone whose pooled feature is not 1280-d; refused before any launch. */
int syn_synergy_losses(syn_handle *h, const float *param /*[B 62]*/, const float *target /*[B 62]*/, const float *pool /*[B 1280]*/, int B,
                       float *scalars /*[2]: LMK_f0 | LMK_pointNet*/, float *per_face /*[3][B]: Param_In | Param_S2 | Param_S1S2*/,
                       double *meter /*nullable: 8 doubles on the device*/, void *stream);

/* ---- backward of the loss head and of its two loss modules (vector-Jacobian products) ---- */

/* The vector-Jacobian product of the loss head of syn_synergy_losses: given what flows into each of the five losses it returns the
 * gradients of the head's two inputs, d_param [B,62] and d_pool [B,1280] (what main_train.py:138 needs at the backbone boundary).
 *   g_scalars[2]     upstream gradients of loss_LMK_f0 and loss_LMK_pointNet          (device)
 *   g_per_face[3][B] upstream gradients of loss_Param_In, loss_Param_S2, loss_Param_S1S2 (device)
 * Both NULL: 1 for the two scalars and 1 / B for each per-face loss, i.e. the gradient of main_train.py:128-132's loss_total.  Exactly
 * one of them NULL is SYN_ERR_INVALID.  One C call enqueues the forward launches again, the two WingLoss counts and the backward's
 * launches; no host synchronisation (but see Scratch).  The head is in the eval() form of the forward (BatchNorm running statistics folded): these are the gradients
 * of the reference model in eval().  No gradients for the MLPs' weights (syn_synergy_losses_backward_weights returns them).  Conventions as torch differentiates the reference: a ReLU
 * output of 0 passes nothing; the max over the 68 points routes to the FIRST point that attains it; the WingLoss rules of
 * syn_wing_loss_backward; a face whose param equals its target has NaN in its rows of d_param / d_pool (sqrt'(0) x 0) and no other
 * face sees it.  fp32: the layers' products, their transposes and the per-face products across faces on the exact-fp32 matrix
 * instruction with the forward's K walk, the rest ordered fused multiply-adds; no floating-point atomics; a face's gradient
 * from the three per-face losses has the same bits alone and at any position of any batch, the two WingLoss terms depend on the batch
 * through their integer counts alone.
 * Scratch: the forward's 35.8 KB per face + 20 KB per face + 690 KB per face of a pass of at most 512 faces, i.e. up to 362 MB from
 * 512 faces on -- twenty times what any other entry point keeps; it stays on the handle until syn_destroy.  Growing to it costs a
 * device-wide synchronisation, a free and an allocation INSIDE the call: only a call that does not grow the scratch is free of host
 * synchronisation (make one call at the largest batch first).  One stream per handle, as syn_refine_landmarks.  Refusals as
 * syn_synergy_losses, decided before any launch with the outputs untouched. */
int syn_synergy_losses_backward(syn_handle *h, const float *param /*[B 62]*/, const float *target /*[B 62]*/, const float *pool /*[B 1280]*/,
                                int B, const float *g_scalars /*nullable [2]*/, const float *g_per_face /*nullable [3][B]*/,
                                float *d_param /*[B 62]*/, float *d_pool /*[B 1280]*/, void *stream);

/* syn_synergy_losses_backward plus the gradients of MLP_for's / MLP_rev's weights: fine-tuning with frozen BatchNorm.
 * d_flat [syn_synergy_flat_count()] has the FLAT layout of syn_load_synergy and receives the gradients of the UNFOLDED tensors: conv
 * weight and bias, BatchNorm weight and bias; the running_mean / running_var slots receive 0.  Every element is written on every call.
 * Per layer y = relu(scale (W x) + shift) with g the gradient at y behind the ReLU mask and before the scale, summed over the faces and
 * (per-point layers) the 68 points: Gx = sum g (x) x, s = sum g; dW = scale Gx, dbias = scale s, dbeta = s, dgamma = rstd (sum_k W Gx +
 * (bias - mean) s) -- no division by gamma.  Upstream conventions and NULL / NULL as syn_synergy_losses_backward; d_param / d_pool are
 * optional here and, when given, have that entry's bits.  The products across faces run on the exact-fp32 matrix instruction (a face's
 * 68 points are 17 whole K steps: no padded row enters a sum), conv5's as ordered fused multiply-adds over faces; no floating-point
 * atomics; faces are added in ascending order, pass after pass, so the bits are a function of the inputs, B and the pass size alone.
 * Scratch: that entry's per-face 55.8 KB + 2.3 KB per face + 7.3 MB of accumulators + (690 + 419) KB per face of a pass of at most 256
 * faces (test knob wgrad_pass), i.e. up to 284 MB; caveats as there.  SYN_ERR_INVALID also for NULL d_flat; refused before any launch. */
int syn_synergy_losses_backward_weights(syn_handle *h, const float *param /*[B 62]*/, const float *target /*[B 62]*/,
                                        const float *pool /*[B 1280]*/, int B, const float *g_scalars /*nullable [2]*/,
                                        const float *g_per_face /*nullable [3][B]*/, float *d_param /*nullable [B 62]*/,
                                        float *d_pool /*nullable [B 1280]*/, float *d_flat /*[syn_synergy_flat_count()]*/, void *stream);

/* Replaces the MLPs' weights from a flat state that lives on the DEVICE (the layout of syn_load_synergy): folded in fp64 and rounded
 * once, as the host does, and repacked into the handle's buffers by one launch on `stream`; no host synchronisation, no download.
 * SYN_ERR_NOT_LOADED unless syn_load_synergy ran once on this handle (the buffers and offsets come from that call). */
int syn_update_synergy_device(syn_handle *h, const float *flat_dev /*[n] device*/, size_t n, void *stream);

/* ---- the loss head's forward under BatchNorm BATCH statistics: the reference in train() (main_train.py:113) ---- */

/* BatchNorm channels of the two MLPs: 3649 = 2243 (forwardDirection.bn1..bn9) + 1406 (reverseDirection.bn1..bn5, bn6_1, bn6_2, bn6_3) */
size_t syn_synergy_bn_channels(void);

/* syn_synergy_losses with every BatchNorm1d of MLP_for / MLP_rev normalising by the statistics of the CURRENT batch:
 *   y = (z - mean) rsqrt(var_biased + 1e-5) gamma + beta,  z = W x + bias,
 * mean / var over all 68 B rows for the per-point layers (conv1..conv5 of both trunks, conv6..conv9 of MLP_for; conv6's statistics
 * are those of the per-point half PLUS the face's per-face half) and over the B faces for the three heads of MLP_rev; the max over a
 * face's 68 points comes after BatchNorm + ReLU.  One call is one replica of nn.DataParallel: the statistics are those of ITS faces.
 * Outputs, loss weights, meter and the WingLoss / ParamLoss conventions are syn_synergy_losses's; the call ends in that entry's one
 * loss launch.  W, bias, gamma, beta are the UNFOLDED tensors of the handle's flat state (syn_load_synergy / syn_update_synergy_device).
 *   batch_stats (nullable) [2][3649]: every BatchNorm's batch mean | biased variance, BatchNorms in the FLAT layout's order
 *   momentum in [0, 1]: running = (1 - momentum) running + momentum stat, the variance in its unbiased form n / (n - 1) (n = 68 B, or B
 *     for the heads), written into the handle's flat state by our launch and re-folded, so that every eval() entry of this handle
 *     (syn_refine_*, syn_landmarks_to_param, syn_synergy_losses*) sees the moved statistics from the next call on; the reference
 *     trains with 0.1.  momentum < 0: the running statistics and every eval() entry stay untouched, bit for bit.
 * fp32: the layer products on the exact-fp32 matrix instruction, K ascending 16 at a time; normalisation in the centred form above;
 * the sums of z and z z in fp64 over fixed blocks of 256 rows (test knob train_rows; the heads: blocks of a sixteenth as many faces,
 * at least 16), folded in ascending block order; no
 * floating-point atomics: the bits are a function of the inputs, B and the block size alone, and a row's z does not depend on its
 * position in the batch.  Stream-ordered, no host synchronisation apart from scratch growth (caveat as syn_refine_landmarks).
 * Scratch: 593 KB per face (z of conv5 materialised: 279 KB; two layer images of 139 KB; conv2's output; the per-face vectors), i.e.
 * 607 MB at 1024 faces; at most 4096 faces per call (2.4 GB).  It stays on the handle until syn_destroy.
 * Refused before any launch with the outputs untouched: SYN_ERR_INVALID for B < 2 (torch: "Expected more than 1 value per channel
 * when training"), B > 4096, NULL pointers, momentum > 1 or NaN, outputs that overlap, a backbone whose pooled feature is not 1280-d;
 * SYN_ERR_NOT_LOADED before syn_load_synergy / syn_load_basis.  There is no backward under batch statistics yet. */
int syn_synergy_losses_train(syn_handle *h, const float *param /*[B 62]*/, const float *target /*[B 62]*/, const float *pool /*[B 1280]*/, int B,
                             float *scalars /*[2]*/, float *per_face /*[3][B]*/, double *meter /*nullable, as syn_synergy_losses*/,
                             float *batch_stats /*nullable [2][3649]*/, float momentum /*0..1, negative: running statistics untouched*/,
                             void *stream);

/* The inverse of syn_update_synergy_device: the handle's flat state, with the running statistics syn_synergy_losses_train has moved,
 * copied device to device on `stream`.  SYN_ERR_NOT_LOADED before syn_load_synergy. */
int syn_export_synergy_flat(syn_handle *h, float *flat_dev /*[n] device*/, size_t n, void *stream);

/* d_pred[e] = g slope sign(pred[e] - target[e]) / n for syn_wing_loss(pred, target): slope = omega / (epsilon + d) for d < omega and 1 for
 * d >= omega with d = |target - pred| in fp32, n = the batch-wide number of elements that took a branch (an integer count, formed on the
 * device by a first launch).  As torch differentiates the reference: d == 0 gives 0; a NaN d is not counted and receives 0, not NaN;
 * d = inf is linear, +-1 / n; every d NaN gives all zeros.  The gradient of `target` is the negative of d_pred.  g: one float on the
 * device, NULL = 1.  fp64 behind the fp32 difference, one rounding; no floating-point sum: the same bits on every call and handle.
 * Scratch, ordering and the refusals of syn_wing_loss; d_pred is untouched by a refused call. */
int syn_wing_loss_backward(syn_handle *h, const float *pred, const float *target, int B, int n_points, float omega, float epsilon,
                           const float *g /*nullable: 1 float on the device*/, float *d_pred /*[B 3 n_points]*/, void *stream);

/* Gradients of syn_param_loss(input, target, mode) for the upstream g [B] (NULL = ones): d_input[b][k] = g[b] diff / (count L[b]) with
 * count = 12 for k < 12 and 50 behind it (mode 0), 50 for k < 50 and nothing (0) for k >= 50 (mode 1); d_target is the negative at the
 * target's own positions (mode 1: target[12 + k] against input[k]; target[:12] receives 0).  L[b] == 0 gives NaN (0 / 0, torch's
 * sqrt'(0) x 0) in that face's gradient and in no other face's.  A face's gradient has the same bits alone and at any position of any
 * batch.  Either output may be NULL, not both.  No scratch.  Refusals as syn_param_loss; the outputs are then untouched. */
int syn_param_loss_backward(syn_handle *h, const float *input /*[B 62]*/, const float *target /*[B 62]*/, int B, int mode,
                            const float *g /*nullable [B]*/, float *d_input /*nullable [B 62]*/, float *d_target /*nullable [B 62]*/,
                            void *stream);

/* CenterCrop(margin, mode='test') of the reference's benchmark loader (utils/ddfa.py:162-243) on uint8 images [B,H,W,C]: the interior
 * [margin, H - margin) x [margin, W - margin) is copied, everything else becomes 0.  margin = 0: a plain copy; 2 margin >= min(H, W): all
 * zeros (what the reference's slices give).  in == out is allowed (any other overlap is not).  SYN_ERR_INVALID for NULL pointers, a
 * dimension <= 0 or margin < 0. */
int syn_center_crop_u8(syn_handle *h, const uint8_t *in /*[B H W C]*/, int B, int H, int W, int C, int margin, uint8_t *out, void *stream);

/* The reference's training transform (main_train.py:199-208: ColorJitter, ToTensor, CenterCrop in its train form, Normalize; utils/ddfa.py
 * and PIL's ImageEnhance) on a uint8 set that lives on the device: output face i is face records[i].src_index of `src`, jittered, cropped,
 * masked and normalised, bit for bit what the reference's loader produces for the same draws.  One launch, one workgroup per output face;
 * the gather by src_index happens in the kernel.
 *   steps      op[j] = 0 skip, 1 brightness, 2 contrast, 3 saturation with factor[j], applied in the order j = 0, 1, 2; repeats allowed.
 *              Each is PIL's blend(degenerate, image, factor) per byte, t = fp32(d) + fp32(factor * fp32(x - d)) with the product and
 *              the sum rounded separately: truncated for 0 <= factor <= 1, otherwise 0 for t <= 0, 255 for t >= 255, truncated between.
 *              d = 0 (brightness); the pixel's grey L = (19595 c0 + 38470 c1 + 7471 c2 + 32768) >> 16 (saturation; channel 0 is the
 *              first byte in memory: the reference hands BGR bytes to PIL as RGB, and so does this); floor((2 sum L + H W) / (2 H W))
 *              over the image as it stands when the step runs (contrast; an integer sum).
 *   crop, mask pixels outside [margin, H - margin) x [margin, W - margin) become 0; mask kind k != 0 zeroes everything outside its box too,
 *              rows x columns: 1 [0, H/2) x [0, W/2); 2 [0, H/2) x [W/2, W); 3 [H/2, H) x [0, W/2); 4 the box of kind 1 (the reference's
 *              rdown repeats lup); 5 all x [0, W/2); 6 all x [W/2, W); 7 [H/4, H - ceil(H/4)) x [W/4, W - ceil(W/4)).  2 margin >= min(H, W): all 0.
 *   out_f32    [B 3 H W]: fp32(fp32(byte - mean) / std), a correctly rounded division; a zeroed pixel is (0 - mean) / std
 *   out_u8     [B H W 3]: the jittered, cropped, masked bytes (what syn_backbone_forward_u8 ingests).  Either output may be NULL, not both.
 * A face's output bits do not depend on B or on its position in the batch.  src and the outputs need no alignment; a face whose first
 * byte is 16-byte aligned is read with 16-byte loads, any other with byte loads.
 * The caller's error, but never an access outside the buffers: a record with src_index outside [0, N), an op above 3 or a mask above 7
 * gives an all-zero face (every byte 0, every float (0 - mean) / std).
 * No scratch, no host synchronisation, asynchronous on `stream`; src, records and the outputs are device pointers.
 * Refused with SYN_ERR_INVALID and the outputs untouched: a NULL h, src or records; both outputs NULL; N, H, W or B <= 0; margin < 0; std
 * 0 or not finite; mean not finite; 3 H W above SYN_TRAIN_TRANSFORM_MAX_FACE_BYTES (the face and its reduction words live in one
 * workgroup's 160 KiB of LDS); an output that overlaps src or the other output. */
typedef struct syn_train_record {
    int32_t src_index;
    float factor[3];
    uint8_t op[3];
    uint8_t mask;
} syn_train_record;
#define SYN_TRAIN_TRANSFORM_MAX_FACE_BYTES 163776          /* 160 KiB - 16 reduction words; 3 H W may not exceed it */
int syn_train_transform_u8(syn_handle *h, const uint8_t *src /*[N H W 3]*/, int N, int H, int W, const syn_train_record *records /*[B]*/, int B,
                           int margin, float mean, float std, float *out_f32 /*nullable [B 3 H W]*/, uint8_t *out_u8 /*nullable [B H W 3]*/,
                           void *stream);

/* ---- introspection (bench / profiling) --------------------------------------------- */

/* Number of kernel launches one per-layer syn_backbone_forward issues. */
int syn_backbone_launch_count(syn_handle *h);

/* Runs one forward with a HIP event recorded on the library's stream after every kernel launch.
 * Returns the number of launches n (<= max_launches) or a negative syn_status; for launch i:
 * feature_of_launch[i] = index into .features the launch completes (1 = fused stem + features.1,
 * 19 = pool + heads, 100 * a + b = one launch covering .features[a] .. [b]), ms_of_launch[i] = event-to-event time, flops_of_launch[i] = algorithmic FLOPs
 * of the layers it covers for the whole batch (no halo / padding work counted).  Synchronises. */
int syn_backbone_profile(syn_handle *h, const uint8_t *img_hwc, int B, int max_launches,
                         int *feature_of_launch, float *ms_of_launch, double *flops_of_launch);

/* One layer of the loaded MobileNetV1 (arch 2 / 3 / 4) on activations the caller supplies, through the launches the forward itself uses
 * (one helper derives the launch arguments for both) -- the hook tests/test_gpu_mobilenet1_layers.py judges every element of every layer with.
 *   layer 0      stem: in = uint8 HWC [B,120,120,3] when in_u8 is set, fp32 CHW [B,3,120,120] otherwise; out = NHWC [B,60,60,c0].
 *   layer 1..13  block layer - 1 (dw2_1 .. dw6): in = NHWC fp32 [B,hin,hin,cin], out = [B,hout,hout,cout].  fused = 1: the one-launch block;
 *                fused = 0: the depthwise and then the pointwise launch, and a non-NULL aux receives the depthwise output [B,hout,hout,cin].
 *   layer 14     pool + heads: in = [B,4,4,pool], out = [B,62], a non-NULL aux receives the pooled feature [B,pool] (fused is ignored).
 * n_in / n_out / n_aux are ELEMENT counts of the three buffers (n_aux = 0 when aux is NULL).  Refused with SYN_ERR_INVALID and a message that
 * names what was expected, before any launch and, for a NULL handle, before a device is touched: a count that differs from what the layer
 * needs, a handle whose arch is not MobileNetV1, layer outside 0..14, B < 1 or B > 65536, fused other than 0 / 1, aux with fused = 1 on a block (the
 * depthwise output never leaves the chip there) or on layer 0, in_u8 on a layer other than 0.  Asynchronous on `stream`; all pointers are device
 * pointers.  c0 = 32 w, pool = 1024 w, block shapes as in DESIGN 5.13 (w = 1, 0.5, 2). */
int syn_mobilenet1_layer(syn_handle *h, int layer, int fused, const void *in, int in_u8, int B, size_t n_in,
                         float *out, size_t n_out, float *aux, size_t n_aux, void *stream);

/* .features[first] .. .features[last] of the loaded mobilenet_v2 (arch 0) on activations the caller supplies -- the hook
 * tests/test_gpu_mobilenet2_spans.py judges every element of every launch with.  The span runs inside the forward's own launch loop, entered
 * at `first` and left at `last`, so the launches are the ones the forward selects for this batch size under the handle's schedule
 * (SYNERGY_HIP_FUSION, SYNERGY_HIP_EARLY_RM, the range verdict, the test knobs); a pair or chain launch that the span cuts is replaced by
 * the single-block launches, as in syn_backbone_profile's per-block mode.
 *   first = 0     in = uint8 HWC crops [B,120,120,3] when in_u8 is set, fp32 CHW crops [B,3,120,120] otherwise; last >= 1 (the stem and
 *                 features.1 share a launch)
 *   first = 2..18 in = the NHWC fp32 input of .features[first], [B,hin,hin,cin]
 *   last <= 18    out = the NHWC output of .features[last], [B,hout,hout,cout]
 *   last = 19     through pool and heads: out = [B,62], a non-NULL aux receives the pool [B,1280] (the hidden-sliced features.17 that the tail
 *                 adds up while staging its input is only reachable this way)
 * Returns the number of launches n, or a negative syn_status; launch_tags[i] = what syn_backbone_profile calls feature_of_launch: 1 (stem +
 * features.1), f (one launch, or the per-layer launches, of .features[f]), 100 a + b (.features[a] .. [b] in one launch, 1517 among them),
 * 19 (pool + heads).  No events are created.  n_in / n_out / n_aux are ELEMENT counts (n_aux = 0 when aux is NULL).  Refused with
 * SYN_ERR_INVALID and a message that names what was expected, before any launch, with `out` untouched: a count that differs from what
 * the span needs, a handle whose arch is not mobilenet_v2, first > last or either outside 0..19 (first = 19 included), first = 1, first = 0
 * with last = 0, in_u8 with first != 0, aux with last != 19, B < 1 or B > 65536, max_tags below the span's layer count (+ 1 with last = 19:
 * the most launches any schedule issues).  Asynchronous on `stream`; all pointers but launch_tags are device pointers; the intermediates
 * live in the handle's workspace (one stream at a time, as the forward). */
int syn_mobilenet2_span(syn_handle *h, int first, int last, const void *in, int in_u8, int B, size_t n_in, float *out, size_t n_out,
                        float *aux, size_t n_aux, int *launch_tags, int max_tags, void *stream);

/* Blocks first .. last of the loaded resnet50 (arch 1) on activations the caller supplies -- the hook tests/test_gpu_resnet50_spans.py judges
 * every element of every launch with.  Block 0 = stem + max-pool, 1..16 = the bottlenecks layer1.0 .. layer4.2, 17 = pool + heads.  The span
 * runs inside the forward's own loop, entered at `first` and left behind `last`, so the launches are the ones the forward selects for this
 * batch size under the handle's SYNERGY_HIP_FUSION, SYNERGY_HIP_RESNET_FUSE, SYNERGY_HIP_RESNET_GEMM, SYNERGY_HIP_RANGE_GUARD, weight
 * verdict and test knobs.  All buffers are plain fp32 NHWC; inside an fp16 x2 forward the hook converts the input to the pair format and
 * the results back (hi + lo is exact: the way out loses nothing).
 *   first = 0      in = uint8 HWC crops [B,120,120,3] when in_u8 is set, fp32 CHW crops [B,3,120,120] otherwise
 *   first = 1..17  in = the input of block `first`, [B,hin,hin,cin] ([B,4,4,2048] for 17)
 *   last <= 16     out = the output of block `last`, [B,hout,hout,cout] ([B,30,30,64] for 0)
 *   last = 17      out = [B,62], a non-NULL aux receives the pool [B,2048]
 *   last = 1..15   the fused launch that ends block `last` (conv_c3f_kernel) also produces conv1 of block last + 1; it is not replaced, and
 *                  a non-NULL aux receives that conv1 output [B,h,h,c1].  Where no fused launch ran (an fp32 handle, SYNERGY_HIP_RESNET_FUSE=0,
 *                  layers 3 / 4) aux is left untouched and SYN_SPAN_AUX_WRITTEN is not set in the return value.
 * Returns the number of launches n, with SYN_SPAN_AUX_WRITTEN or-ed in when aux (last <= 15) was written, or a negative syn_status.
 * launch_tags[i] = 1000 x block + the code of the KERNEL VARIANT of launch i, as the launcher that chose it reports it:
 *     1  resnet_stem_kernel (direct)        3  resnet_stem_mfma_kernel        4  resnet_stem_mfma_kernel with the max-pool epilogue
 *     5  maxpool3x3s2_kernel               90  pool_fc_generic_kernel        60  conv_lp_kernel DUAL (conv3 + stride-2 downsample branch)
 *    10 + MT  conv_kernel<MT,4> (exact fp32 MFMA; MT = 1, 2, 4)
 *    20 + MT  conv_f16x2_kernel<MT,4> (64-bit addressing; MT = 1, 2)             30 + MT  conv_h2s_kernel<MT,4,2> (MT = 1, 2)
 *    40 + 2 [MTW = 4] + [frag]  conv_lt_kernel<MTW,frag> (MTW = 2, 4)            50 + 2 [MTW = 4] + [frag]  conv_lp_kernel<MTW,frag>
 *   100 + 10 shape + 4 [DS] + 2 [C2F] + [identity in pairs]  conv_c3f_kernel; shape 0 = <KS3 2, NT1 4> (layer 1), 1 = <2, 8> (layer 1 ->
 *        layer 2), 2 = <4, 8> (layer 2); DS = the downsample branch in the kernel (layer1.0), C2F = conv2 in front
 * With the range guard armed the span resets and fills the status array as the forward does; the slots of guarded tensors the span did
 * not produce read 1 like the unguarded ones, so syn_backbone_range_status returns the maxima of the tensors the span produced.
 * n_in / n_out / n_aux are ELEMENT counts (n_aux = 0 when aux is NULL).  Refused with SYN_ERR_INVALID and a message that names what was
 * expected, before any launch, with `out` untouched: a count that differs from what the span needs, a handle whose arch is not resnet50,
 * first > last or either outside 0..17, in_u8 with first != 0, aux with last = 0 or 16, B < 1 or B > 65536, max_tags below the span's
 * per-layer launch count (2 for block 0, 3 per bottleneck, 4 with a downsample branch, 1 for block 17).  Asynchronous on `stream`; all
 * pointers but launch_tags are device pointers; the intermediates live in the handle's workspace (one stream at a time, as the forward). */
#define SYN_SPAN_AUX_WRITTEN 0x10000
int syn_resnet50_span(syn_handle *h, int first, int last, const void *in, int in_u8, int B, size_t n_in, float *out, size_t n_out,
                      float *aux, size_t n_aux, int *launch_tags, int max_tags, void *stream);

/* One block of the loaded GhostNet (arch 6) on activations the caller supplies, through exactly the launches the forward uses for that
 * block (one helper derives the launch arguments for both) -- the hook tests/test_gpu_ghostnet.py judges every block with.
 *   block 0..15  bottleneck blocks.0.0 .. blocks.8.3: in = NHWC fp32 [B,hin,hin,cin], out = [B,hout,hout,cout]; on a block with
 *                squeeze-and-excite (3, 4, 9, 10, 11, 13, 15) a non-NULL aux receives the gate [B,mid]
 *   block 16     blocks.9.0 (ConvBnAct): in = [B,4,4,160], out = [B,4,4,960]
 *   block 17     pool + conv_head + ReLU + heads: in = [B,4,4,960], out = [B,62], a non-NULL aux receives the pooled feature [B,1280]
 *   block 18     conv_stem + bn1 + ReLU, the launch the forward makes before block 0: in = normalised fp32 crops NCHW [B,3,120,120],
 *                out = [B,60,60,16]; no aux, `fused` selects nothing
 * fused = 1: the GhostModules of the block that have a fused launch use it; fused = 0: one launch per layer.  n_in / n_out / n_aux are
 * ELEMENT counts (n_aux = 0 when aux is NULL).  Refused with SYN_ERR_INVALID and a message that names what was expected, before any
 * launch, with `out` untouched: a count that differs from what the block needs, a handle whose arch is not ghostnet, block outside
 * 0..18, B < 1 or B > 65536, fused other than 0 / 1, aux on a block that has neither gate nor pool.  Asynchronous on `stream`; all
 * pointers are device pointers; the block's intermediates live in the handle's workspace (one stream at a time, as the forward). */
int syn_ghostnet_block(syn_handle *h, int block, int fused, const float *in, int B, size_t n_in,
                       float *out, size_t n_out, float *aux, size_t n_aux, void *stream);

/* One block of the loaded ResNeSt-50 (arch 8) on activations the caller supplies, through exactly the launches the forward uses for that
 * block (one helper derives the launch arguments for both) -- the hook tests/test_gpu_resnest.py judges every block with.
 *   block 0      stem (three 3x3 convolutions) + max pool: in = normalised fp32 crops [B,120,120,3] (HWC), out = [B,30,30,64]
 *   block 1..16  bottlenecks layer1.0 .. layer4.2: in = NHWC fp32 [B,hin,hin,cin], out = [B,hout,hout,4C]; a non-NULL aux receives the
 *                attention [B,2C] in fc2's order (radix half 0 | radix half 1)
 *   block 17     pool + heads: in = [B,4,4,2048], out = [B,62], a non-NULL aux receives the pool [B,2048]
 * fused = 1: conv3 (and the downsample convolution of layer2.0 / 3.0) build their operands in LDS; fused = 0: one launch per layer.
 * n_in / n_out / n_aux are ELEMENT counts (n_aux = 0 when aux is NULL).  Refused with SYN_ERR_INVALID and a message that names what was
 * expected, before any launch, with `out` untouched: a count that differs from what the block needs, a handle whose arch is not
 * resnest50, block outside 0..17, B < 1 or B > 65536, fused other than 0 / 1, aux on block 0.  Asynchronous on `stream`; all pointers
 * are device pointers; the block's intermediates live in the handle's workspace (one stream at a time, as the forward). */
int syn_resnest50_block(syn_handle *h, int block, int fused, const float *in_nhwc, int B, size_t n_in,
                        float *out, size_t n_out, float *aux, size_t n_aux, void *stream);

/* One block of the loaded resnet18 / resnet34 (arch 10 / 11) on activations the caller supplies, through exactly the launches the forward
 * uses for that block (one helper derives the launch arguments for both) -- the hook tests/test_gpu_resnet_basic.py judges every block with.
 *   block 0          stem + max pool: in = normalised fp32 crops [B,3,120,120] (NCHW, as syn_backbone_forward takes them), out = [B,30,30,64]
 *   block 1..8 / 16  BasicBlocks layer1.0 .. layer4.1 / layer4.2: in = NHWC fp32 [B,hin,hin,cin], out = [B,hout,hout,C]
 *   block 9 / 17     pool + heads: in = [B,4,4,512], out = [B,62]
 * fused = 1: the LDS-tiled convolutions (the downsample inside conv1 on layer2.0 / 3.0 / 4.0); fused = 0: one launch per layer, taps from
 * global memory.  n_in / n_out are ELEMENT counts.  Refused with SYN_ERR_INVALID and a message that names what was expected, before any
 * launch, with `out` untouched: a count that differs from what the block needs, a handle whose arch is neither resnet18 nor resnet34, a
 * block outside the range, B < 1 or B > 65536, fused other than 0 / 1.  Asynchronous on `stream`; all pointers are device pointers; the
 * block's intermediates live in the handle's workspace (one stream at a time, as the forward). */
int syn_resnet_basic_block(syn_handle *h, int block, int fused, const float *in_nhwc, int B, size_t n_in, float *out, size_t n_out,
                           void *stream);

/* The dense reconstruction (transform = 1) into a pitched output with HIP events around its kernels, on the default stream;
 * synchronises.  ms2[0] = per-face prologue, ms2[1] = the contraction + pose epilogue + mesh stores -- the HBM-write-bound kernel
 * of the path (B * 3 * n_vert * 4 bytes).  Arguments as syn_reconstruct_pitched. */
int syn_reconstruct_profile(syn_handle *h, const float *param, int B, const float *roi, float *out, int row_pitch, int pad_writable,
                            float *ms2);

/* Algorithmic FLOPs per face of the whole backbone / of its pointwise (MFMA) convolutions. */
double syn_backbone_flops_per_face(void);
double syn_pointwise_flops_per_face(void);

#ifdef __cplusplus
}
#endif
#endif /* SYNERGY_HIP_H */
