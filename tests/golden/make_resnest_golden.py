"""Generate tests/golden/resnest50_outputs.npz by running the REAL reference ResNeSt-50 module (authoring container only).

    python tests/golden/make_resnest_golden.py

Follows make_ghostnet_golden.py: the reference's own resnest50() (backbone_nets/ResNeSt/resnest.py:33-41, torch-only, importable as-is)
loaded strictly with synth.make_resnest50_state(seed), run on synth.normalize_crops(resnest_cases.golden_crops()).  Recorded: out62, the
pool [2,2048], per block (stem + max pool, then the 16 bottlenecks) the output's mean and abs-max per face, per bottleneck the
attention's min / max / mean per face and its share inside (0.05, 0.95), the seeds, and the module's state_dict() key names with their
shapes.  No weights."""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..', '..')))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..')))

from synergynet_amd import synth          # noqa: E402
from oracle import ref_loader             # noqa: E402
import resnest_cases as rc                # noqa: E402


def reference_module():
    sys.path.insert(0, ref_loader.REF_ROOT)
    try:
        m = importlib.import_module('backbone_nets.ResNeSt.resnest')
    finally:
        sys.path.remove(ref_loader.REF_ROOT)
    return m.resnest50().eval()


def run_reference(seed, x):
    """dict of everything recorded, from the reference module with the synthetic weights of `seed`."""
    net = reference_module()
    own = net.state_dict()
    sd = synth.make_resnest50_state(seed)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})      # strict: the key sets are equal
    blocks, atts = {}, {}
    net.maxpool.register_forward_hook(lambda m_, i, o: blocks.__setitem__(0, o.clone()))
    for idx, (name, *_r) in enumerate(rc.BLOCKS):
        mod = net.get_submodule(name)
        mod.register_forward_hook(lambda m_, i, o, idx=idx: blocks.__setitem__(idx + 1, o.clone()))
        mod.conv2.rsoftmax.register_forward_hook(lambda m_, i, o, idx=idx: atts.__setitem__(idx, o.flatten(1).clone()))
    with torch.no_grad():
        out, pool = net(torch.from_numpy(x))
    keys = list(own.keys())
    shapes = np.zeros((len(keys), 4), dtype=np.int64)
    ndim = np.zeros(len(keys), dtype=np.int64)
    for i, k in enumerate(keys):
        s = tuple(own[k].shape)
        ndim[i] = len(s)
        shapes[i, :len(s)] = s
    return {'out62': out.numpy(), 'pool': pool.flatten(1).numpy(), 'keys': np.array(keys), 'shapes': shapes, 'ndim': ndim,
            'block_mean': np.stack([blocks[i].mean(dim=(1, 2, 3)).numpy() for i in range(17)]),
            'block_absmax': np.stack([blocks[i].abs().amax(dim=(1, 2, 3)).numpy() for i in range(17)]),
            'att_min': np.stack([atts[i].min(dim=1).values.numpy() for i in range(16)]),
            'att_max': np.stack([atts[i].max(dim=1).values.numpy() for i in range(16)]),
            'att_mean': np.stack([atts[i].mean(dim=1).numpy() for i in range(16)]),
            'att_inside': np.stack([((atts[i] > 0.05) & (atts[i] < 0.95)).float().mean(dim=1).numpy() for i in range(16)])}


def main():
    torch.manual_seed(0)
    x = synth.normalize_crops(rc.golden_crops())
    rec = run_reference(rc.SEED, x)
    rec.update({'seed': np.array(rc.SEED), 'crops_seed': np.array(rc.CROPS_SEED)})
    print('out[0,:4] =', rec['out62'][0, :4], 'pool non-zero', float((rec['pool'] != 0).mean()))
    print('block abs-max', rec['block_absmax'].max(axis=1).round(2))
    print('attention inside (0.05, 0.95)', rec['att_inside'].min(axis=1).round(3))
    np.savez_compressed(rc.GOLDEN, **rec)
    print('wrote', rc.GOLDEN, os.path.getsize(rc.GOLDEN), 'bytes')


if __name__ == '__main__':
    main()
