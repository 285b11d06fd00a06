"""GPU box: what a training batch costs when it is born on the device.

    python tools/augment_bench.py [--batches 128,1024] [--steps 10] [--warmup 5] [--set 8192]

A resident uint8 set of `--set` 120 x 120 crops (8192: 354 MB, more than the Infinity Cache holds) and, per batch size and output kind,
`--inner` record batches already on the device, each with its own random source indices, orders, factors and masks (prob 0.01, as the
reference trains).  One step = the `--inner` launches of syn_train_transform_u8 back to back between two device events; after a warm-up
the median / min / max of `--steps` steps, divided by `--inner`, is the time of one launch.  Beside it: the bytes the launch has to
move (the face read once, the outputs written once) per second, next to the 5.2 TB/s measured for whole-line stores; what
the host spends drawing and checking the records of one batch (python, sequential by construction: the reference's draw order); and the
CPU yardstick of this box -- the numpy RESTATEMENT of the transform (tests/augment_cases.py), one thread, per crop.  The reference's own
PIL transform is not on this box: its 619 us per crop was measured on the authoring machine's CPU (one thread, one run of 500 calls).
Prints one JSON line per (batch size, output kind) and one for the CPU figures.  No acceptance threshold."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import augment_cases as ac                                # noqa: E402
from synergynet_amd import abi, augment, synth            # noqa: E402
from synergynet_amd.synergy3DMM import SynergyNet         # noqa: E402

STORE_BOUND_TBS = 5.2                                     # whole-line stores in isolation
REFERENCE_US_PER_CROP = 619.0                             # the reference's transform through PIL, authoring machine, one thread, 500 calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='128,1024')
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--set', type=int, default=8192)
    a = ap.parse_args()
    if a.steps < 10:
        ap.error('--steps: at least 10 (a median of fewer says little)')
    m = SynergyNet(device='cuda:0', pack=synth.make_3dmm(), backbone_state=synth.make_backbone_state())
    H = W = 120
    face = 3 * H * W
    crops = torch.randint(0, 256, (a.set, H, W, 3), dtype=torch.uint8, device='cuda')
    rs, pr = np.random.RandomState(0), random.Random(0)
    device = torch.cuda.get_device_name(0)
    for B in [int(b) for b in a.batches.split(',')]:
        t0 = time.perf_counter()
        recs = []
        for _ in range(a.inner):
            r = augment.draw_records(B, np_random=rs, py_random=pr)
            r['src_index'] = rs.randint(0, a.set, B)
            recs.append(augment.check_records(r, a.set))
        host_us = (time.perf_counter() - t0) / a.inner * 1e6
        drec = [torch.from_numpy(r.view(np.uint8).reshape(B, 20)).cuda() for r in recs]
        f32 = torch.empty((B, 3, H, W), dtype=torch.float32, device='cuda')
        u8 = torch.empty((B, H, W, 3), dtype=torch.uint8, device='cuda')
        kinds = (('f32', f32.data_ptr(), None, face + 4 * face), ('u8', None, u8.data_ptr(), 2 * face), ('both', f32.data_ptr(), u8.data_ptr(), 6 * face))
        us = {k[0]: [] for k in kinds}
        for it in range(a.warmup + a.steps):
            for name, pf, pu, _ in kinds:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for d in drec:
                    abi.check(m._lib.syn_train_transform_u8(m._h, crops.data_ptr(), a.set, H, W, d.data_ptr(), B, 5, 127.5, 128.0, pf, pu, m._stream()))
                e1.record()
                e1.synchronize()
                if it >= a.warmup:
                    us[name].append(e0.elapsed_time(e1) * 1e3 / a.inner)
        for name, _, _, bytes_per_face in kinds:
            v = us[name]
            med = statistics.median(v)
            tbs = bytes_per_face * B / (med * 1e-6) / 1e12
            print(json.dumps(dict(B=B, out=name, us_per_launch=round(med, 2), us_min=round(min(v), 2), us_max=round(max(v), 2),
                                  us_per_face=round(med / B, 4), bytes_per_face=bytes_per_face, tb_per_s=round(tbs, 3),
                                  share_of_store_bound=round(tbs / STORE_BOUND_TBS, 3), host_draw_check_us_per_batch=round(host_us, 1),
                                  steps=a.steps, warmup=a.warmup, inner=a.inner, set=a.set, device=device)), flush=True)
    # the CPU yardstick of this box: the numpy restatement, one thread
    img = crops[0].cpu().numpy()
    r = augment.draw_records(20, np_random=rs, py_random=pr)
    t = []
    for i in range(20):
        t0 = time.perf_counter()
        ac.train_transform(img, r['op'][i], r['factor'][i], int(r['mask'][i]), 5, 127.5, 128.0)
        t.append((time.perf_counter() - t0) * 1e6)
    print(json.dumps(dict(cpu='numpy restatement of the transform (tests/augment_cases.py), this box, one thread, median of 20 crops',
                          restatement_us_per_crop=round(statistics.median(t), 1),
                          reference_us_per_crop=REFERENCE_US_PER_CROP,
                          reference_measured='the reference through PIL on the authoring machine (not this box), one thread, one run of 500 calls')),
          flush=True)


if __name__ == '__main__':
    main()
