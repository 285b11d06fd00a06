"""GPU box: what BatchNorm batch statistics cost the loss head's forward.

    python tools/loss_train_bench.py [--batches 2,128,1024] [--steps 10] [--warmup 5]

Two steps alternate in ONE process after a warm-up, device events around each, median / min / max of the steps, on param / pool / target
that are already on the device:
  eval   syn_synergy_losses        (running statistics folded, one workgroup per face: the parent's behaviour and the yardstick)
  train  syn_synergy_losses_train  (layer by layer over the 68 B rows, a statistics launch behind every product; momentum 0.1, so the
                                    running update and the re-fold are part of the step)
Prints one JSON line per batch size, with the bytes of z the layer-by-layer head writes and reads per face.  There is no acceptance
threshold: nobody has measured a layer-by-layer head on this device before."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from synergynet_amd import synth                          # noqa: E402
from synergynet_amd.synergy3DMM import SynergyNet         # noqa: E402

# columns of z per point: both trunks (conv1 .. conv5) and conv6 .. conv9 of MLP_for (conv9's image has 4 columns); every z is written
# once by its product and read once by the next product (z2 of MLP_for twice: conv3 and conv6), z5 by the max
Z_COLUMNS = 2 * (64 + 64 + 64 + 128 + 1024) + 512 + 256 + 128 + 4
Z_BYTES_PER_FACE = 68 * 4 * (2 * Z_COLUMNS + 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='2,128,1024')
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=5)
    a = ap.parse_args()
    if a.steps < 10:
        ap.error('--steps: at least 10 (a median of fewer says little)')
    m = SynergyNet(device='cuda:0', pack=synth.make_3dmm(), backbone_state=synth.make_backbone_state())
    m.load_synergy_state(synth.make_synergy_state())
    for B in [int(b) for b in a.batches.split(',')]:
        param = torch.from_numpy(synth.make_params(B, seed=B)).cuda()
        target = torch.from_numpy(synth.make_params(B, seed=B + 1)).cuda()
        pool = torch.rand((B, 1280), device='cuda')
        steps = (('eval', lambda: m._losses(param, pool, target)), ('train', lambda: m._losses_train(param, pool, target, 0.1)))
        ms = {name: [] for name, _ in steps}
        for it in range(a.warmup + a.steps):
            for name, fn in steps:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if it >= a.warmup:
                    ms[name].append(e0.elapsed_time(e1))
        med = {name: statistics.median(v) for name, v in ms.items()}
        rec = dict(B=B, steps=a.steps, warmup=a.warmup, device=torch.cuda.get_device_name(0))
        for name, v in ms.items():
            rec[name] = dict(ms_per_step=round(med[name], 4), ms_min=round(min(v), 4), ms_max=round(max(v), 4))
        rec['train_over_eval'] = round(med['train'] / med['eval'], 2)
        rec['z_bytes_per_face'] = Z_BYTES_PER_FACE
        rec['z_megabytes'] = round(Z_BYTES_PER_FACE * B / 1e6, 1)
        print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
