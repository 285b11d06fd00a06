"""GPU box: HIP-event time of the synergy refinement (syn_refine_landmarks = MLP_for, syn_landmarks_to_param = MLP_rev) next to
syn_backbone_forward_u8 at the same batch in the same process.  Warm-up, then the median of `iters` single calls each.
usage: python tools/time_synergy.py [iters]        (batches 128 and 1024; one JSON line per batch)"""
import json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from synergynet_amd import synth
from synergynet_amd.synergy3DMM import SynergyNet
it = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 30
FLOP_FOR, FLOP_REV = 2 * 25.0e6, 2 * 9.6e6          # per face, conv6's per-face columns hoisted
PEAK_FP32_MFMA = 157.3e12                           # v_mfma_f32_16x16x4_f32, whole chip
m = SynergyNet(device='cuda:0', pack=synth.make_3dmm(), backbone_state=synth.make_backbone_state())
m.load_synergy_state(synth.make_synergy_state())


def median_us(fn):
    for _ in range(5): fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(it):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(ts)


for B in (128, 1024):
    crops = torch.from_numpy(synth.make_crops(B, seed=3)).cuda()
    param, pool = m.forward_crops_u8(crops, return_pool=True)
    lr = m.refine_landmarks(param, pool)
    t_bb = median_us(lambda: m.forward_crops_u8(crops, return_pool=True))
    t_for = median_us(lambda: m.refine_landmarks(param, pool))
    t_rev = median_us(lambda: m.landmarks_to_param(lr))
    print(json.dumps(dict(B=B, iters=it, backbone_u8_us=round(t_bb, 1), refine_landmarks_us=round(t_for, 1), landmarks_to_param_us=round(t_rev, 1),
                          both_over_backbone=round((t_for + t_rev) / t_bb, 3),
                          refine_share_of_fp32_mfma_peak=round(FLOP_FOR * B / (t_for * 1e-6) / PEAK_FP32_MFMA, 3),
                          rev_share_of_fp32_mfma_peak=round(FLOP_REV * B / (t_rev * 1e-6) / PEAK_FP32_MFMA, 3),
                          both_share_of_fp32_mfma_peak=round((FLOP_FOR + FLOP_REV) * B / ((t_for + t_rev) * 1e-6) / PEAK_FP32_MFMA, 3))))
