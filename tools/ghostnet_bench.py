"""GPU box: the GhostNet backbone, fused schedule (one launch per GhostModule on the 15^2, 8^2 and 4^2 maps) against the per-layer
schedule, alternating in ONE process after a warm-up; median of the steps.  forward_crops_u8 only (uint8 crops already on the device).

    python tools/ghostnet_bench.py [--batches 1,32,128,1024] [--steps 20] [--warmup 5] [--per-launch]

Prints one JSON line per batch size: faces/s, ms per step, TFLOP/s and the fraction of the 155 TFLOP/s the fp32-input MFMA was
measured at, for both schedules; --per-launch adds the microseconds of every launch (syn_backbone_profile; launch codes 0 = stem,
100 (block + 1) + step with step 0 ghost1 (primary, or the fused module), 1 ghost1 cheap, 2 conv_dw, 3 SE mean, 4 SE reduce,
5 SE expand, 6 shortcut depthwise, 7 shortcut 1x1, 8 ghost2 (primary, or fused), 9 ghost2 cheap; 1700 ConvBnAct; 1800 pool,
1801 conv_head, 1802 heads)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from synergynet_amd import synth                          # noqa: E402
from synergynet_amd.synergy3DMM import SynergyNet         # noqa: E402

PEAK_TF = 155.0
SCHEDULES = (('fused', 1), ('per_layer', 0))      # syn_set_schedule codes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='1,32,128,1024')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--per-launch', action='store_true')
    a = ap.parse_args()
    if a.steps < 10:
        ap.error('--steps: at least 10 (a median of fewer says little)')
    m = SynergyNet(device='cuda:0', pack=synth.make_3dmm(4321, n_vert=700), backbone_state=synth.make_ghostnet_state(2031), arch='ghostnet')
    lib, h = m._lib, m._h
    flops = lib.syn_ghostnet_flops_per_face()
    for B in [int(b) for b in a.batches.split(',')]:
        crops = torch.from_numpy(synth.make_crops(min(B, 64), seed=B)).cuda().repeat((B + 63) // 64, 1, 1, 1)[:B].contiguous()
        ms = {name: [] for name, _ in SCHEDULES}
        for it in range(a.warmup + a.steps):
            for name, code in SCHEDULES:
                prev = lib.syn_set_schedule(h, code)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                m.forward_crops_u8(crops)
                e1.record()
                e1.synchronize()
                lib.syn_set_schedule(h, prev)
                if it >= a.warmup:
                    ms[name].append(e0.elapsed_time(e1))
        rec = dict(arch='ghostnet', B=B, steps=a.steps, warmup=a.warmup, gflop_per_face=flops / 1e9, device=torch.cuda.get_device_name(0))
        for name, code in SCHEDULES:
            med = statistics.median(ms[name])
            tf = flops * B / (med * 1e-3) / 1e12
            rec[name] = dict(ms_per_step=round(med, 4), ms_min=round(min(ms[name]), 4), ms_max=round(max(ms[name]), 4),
                             faces_per_s=round(B / (med * 1e-3)), tflops=round(tf, 3), frac_of_155tf=round(tf / PEAK_TF, 5))
        rec['fused_over_per_layer'] = round(rec['fused']['ms_per_step'] / rec['per_layer']['ms_per_step'], 4)
        if a.per_launch:
            for name, code in SCHEDULES:
                prev = lib.syn_set_schedule(h, code)
                cap = lib.syn_backbone_launch_count(h)
                feat, t, fl = np.zeros(cap, np.int32), np.zeros(cap, np.float32), np.zeros(cap, np.float64)
                runs = []
                for _ in range(5):
                    n = lib.syn_backbone_profile(h, crops.data_ptr(), B, cap, feat.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p),
                                                 fl.ctypes.data_as(C.c_void_p))
                    assert n == cap, lib.syn_last_error()
                    runs.append(t[:n].copy())
                lib.syn_set_schedule(h, prev)
                us = np.median(np.stack(runs), axis=0) * 1e3
                rec[name]['launches'] = int(cap)
                rec[name]['per_launch_us'] = {int(f): round(float(u), 1) for f, u in zip(feat[:n], us)}
        print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
