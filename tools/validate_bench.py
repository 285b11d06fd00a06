"""GPU box: what the loss stage of SynergyNet.forward(input, target) adds to the graph it scores.

    python tools/validate_bench.py [--batches 1,128,1024] [--steps 10] [--warmup 5]

Three steps alternate in ONE process after a warm-up, device events around each, median of the steps:
  graph    forward_synergy(x) + reconstruct(target, dense=False): the launches forward needs before it can score anything -- backbone, both
           sets of landmarks, MLP_for, MLP_rev -- through entry points that predate the losses
  forward  forward(x, target): the same launches behind one C call, plus the one loss launch
  metered  forward(x, target, meter=...): ... which also adds the batch to the device-side meter
Prints one JSON line per batch size; `added_us` = forward - graph and `metered_added_us` = metered - graph are what the loss stage costs
(they can come out negative at small batches: forward issues its launches from one C call, the graph step from four Python methods)."""
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
    meter = torch.zeros(8, dtype=torch.float64, device='cuda')
    for B in [int(b) for b in a.batches.split(',')]:
        crops = synth.make_crops(min(B, 64), seed=B)
        x = torch.from_numpy(synth.normalize_crops(crops)).cuda().repeat((B + 63) // 64, 1, 1, 1)[:B].contiguous()
        target = torch.from_numpy(synth.make_params(B, seed=B + 1)).cuda()

        def graph():
            m.forward_synergy(x)
            m.reconstruct(target, dense=False)
        steps = (('graph', graph), ('forward', lambda: m.forward(x, target)), ('metered', lambda: m.forward(x, target, meter=meter)))
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
        rec['added_us'] = round((med['forward'] - med['graph']) * 1e3, 1)
        rec['metered_added_us'] = round((med['metered'] - med['graph']) * 1e3, 1)
        rec['added_over_graph'] = round((med['metered'] - med['graph']) / med['graph'], 4)
        print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
