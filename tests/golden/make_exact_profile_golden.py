"""Generate tests/golden/exact_profile_golden.npz from THIS project's library (needs the GPU; nothing comes from the reference).

    python tests/golden/make_exact_profile_golden.py [output.npz]

For the four exact-fp32 families -- MobileNetV1 at its three widths, GhostNet, ResNeSt-50, resnet18 and resnet34 -- and the schedules 0
(per layer) and 1 (fused) of syn_set_schedule: what syn_backbone_profile returns for one forward of two faces
(backbone_blob_cases.launch_profile): the launch codes (feature_of_launch), the algorithmic FLOPs of every launch (flops_of_launch) and
syn_backbone_launch_count.  Times are not recorded.  The weights do not matter to a launch list; they are synth's, seed 3."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..', '..')))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..')))

from synergynet_amd import synth                         # noqa: E402
from synergynet_amd.synergy3DMM import SynergyNet        # noqa: E402
import backbone_blob_cases as bc                         # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else bc.PROFILE
    pack = synth.make_3dmm(4321, n_vert=700)
    crops = torch.from_numpy(bc.profile_crops()).cuda()
    rec = {'batch': np.array(bc.PROFILE_BATCH), 'archs': np.array(bc.EXACT_ARCHS), 'schedules': np.array(bc.SCHEDULES)}
    for arch in bc.EXACT_ARCHS:
        m = SynergyNet(device='cuda:0', pack=pack, backbone_state=bc.make_state(arch), arch=arch)
        for sched in bc.SCHEDULES:
            count, codes, flops = bc.launch_profile(m, crops, sched)
            print(f'{arch:13s} schedule {sched}: launch_count {count:3d}, profiled {codes.size:3d}, {flops.sum() / bc.PROFILE_BATCH / 1e9:.4f} GFLOP / face',
                  flush=True)
            rec[f'{arch}_s{sched}_count'] = np.array(count)
            rec[f'{arch}_s{sched}_codes'] = codes
            rec[f'{arch}_s{sched}_flops'] = flops
        del m
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **rec)
    print('wrote', out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main()
