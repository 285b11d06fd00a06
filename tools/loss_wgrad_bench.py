"""GPU box: what the weight gradients add to the loss head's backward.

    python tools/loss_wgrad_bench.py [--batches 1,128,1024] [--steps 10] [--warmup 5]

Two steps alternate in ONE process after a warm-up, device events around each, median of the steps, on param / pool / target that are
already on the device:
  backward          syn_synergy_losses_backward          (d param, d pool: the parent's behaviour and the yardstick)
  backward_weights  syn_synergy_losses_backward_weights  (the same launches, the weight products across faces after every pass, the
                                                          launch that writes d_flat)
Prints one JSON line per batch size.  There is no acceptance threshold.  The expectation to hold the ratio against is derived, not
measured: the weight products are as many FLOPs as the data-gradient products, so tiled like them they would add 30 to 50 % to the
backward; much more means the reduction across faces is short of parallelism or of operand reuse."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from synergynet_amd import synth                          # noqa: E402
from synergynet_amd.synergy3DMM import SynergyNet         # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='1,128,1024')
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
        steps = (('backward', lambda: m._losses_backward(param, pool, target)),
                 ('backward_weights', lambda: m._losses_backward_weights(param, pool, target)))
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
        rec['weights_over_backward'] = round(med['backward_weights'] / med['backward'], 2)
        print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
