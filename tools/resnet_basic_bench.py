"""GPU box: the resnet18 / resnet34 backbones, LDS-tiled schedule (a workgroup stages a band of input rows with its halo once in LDS;
conv1 of layer2.0 / 3.0 / 4.0 also produces the downsample) against the per-layer schedule (taps from global memory, the downsample a
launch of its own), alternating in ONE process after a warm-up; median of the steps.  forward_crops_u8 only (uint8 crops already on the
device -> 62 parameters).

    python tools/resnet_basic_bench.py [--archs resnet18,resnet34] [--batches 1024,128,32,1] [--steps 10] [--warmup 3] [--per-launch]

Prints one JSON line per arch and batch size: faces/s, ms per step, TFLOP/s (syn_resnet_basic_flops_per_face) and the fraction of the 155
TFLOP/s the fp32-input MFMA was measured at, for both schedules; --per-launch adds the microseconds of every launch (syn_backbone_profile;
launch codes 0 the stem, 1 the max pool; 100 block + step with block 1.. = layer1.0 .. and step 0 conv1 (with the downsample when
LDS-tiled), 1 the downsample, 2 conv2; 100 (blocks + 1) pool + heads), the TFLOP/s of every launch, and `conv3x3_tflops`: the 3x3 launches together."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from synergynet_amd import synth                                    # noqa: E402
from synergynet_amd.synergy3DMM import ARCH_IDS, SynergyNet         # noqa: E402

PEAK_TF = 155.0
SCHEDULES = (('lds', 1), ('per_layer', 0))      # syn_set_schedule codes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--archs', default='resnet18,resnet34')
    ap.add_argument('--batches', default='1024,128,32,1')
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--per-launch', action='store_true')
    a = ap.parse_args()
    if a.steps < 10:
        ap.error('--steps: at least 10 (a median of fewer says little)')
    pack = synth.make_3dmm(4321, n_vert=700)
    for arch in a.archs.split(','):
        m = SynergyNet(device='cuda:0', pack=pack, backbone_state=synth.make_resnet_basic_state(arch, 3187), arch=arch)
        lib, h = m._lib, m._h
        flops = lib.syn_resnet_basic_flops_per_face(ARCH_IDS[arch])
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
            rec = dict(arch=arch, B=B, steps=a.steps, warmup=a.warmup, gflop_per_face=flops / 1e9, device=torch.cuda.get_device_name(0))
            for name, code in SCHEDULES:
                med = statistics.median(ms[name])
                tf = flops * B / (med * 1e-3) / 1e12
                rec[name] = dict(ms_per_step=round(med, 4), ms_min=round(min(ms[name]), 4), ms_max=round(max(ms[name]), 4),
                                 faces_per_s=round(B / (med * 1e-3)), tflops=round(tf, 3), frac_of_155tf=round(tf / PEAK_TF, 5))
            rec['lds_over_per_layer'] = round(rec['lds']['ms_per_step'] / rec['per_layer']['ms_per_step'], 4)
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
                    f_, fl_ = feat[:n], fl[:n]
                    conv = (f_ >= 100) & (f_ != f_.max()) & (f_ % 100 != 1)      # conv1 (with the downsample when LDS-tiled) and conv2
                    rec[name]['launches'] = int(cap)
                    rec[name]['per_launch_us'] = {int(f): round(float(u), 1) for f, u in zip(f_, us)}
                    rec[name]['per_launch_tflops'] = {int(f): round(float(x / (u * 1e-6) / 1e12), 1) for f, u, x in zip(f_, us, fl_) if x > 0}
                    rec[name]['conv3x3_tflops'] = round(float(fl_[conv].sum() / (us[conv].sum() * 1e-6) / 1e12), 2)
            print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
