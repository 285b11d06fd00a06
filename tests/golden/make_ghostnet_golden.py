"""Generate tests/golden/ghostnet_outputs.npz by running the REAL reference GhostNet module (authoring container only).

    python tests/golden/make_ghostnet_golden.py

Follows make_mobilenet1_golden.py: the reference's own ghostnet() (backbone_nets/ghostnet_backbone.py:236-266, torch-only, importable
as-is) loaded strictly with synth.make_ghostnet_state(seed), run on synth.normalize_crops(synth.make_crops(2, seed)).  Recorded: out102,
the act2 output [2,1280] (forward hook), per bottleneck and for blocks.9.0 the output's mean and abs-max per face, every SE gate's
min / max / mean per face, the seeds, and the module's state_dict() key names with their shapes."""
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
import ghostnet_cases as gc               # noqa: E402


def reference_module():
    sys.path.insert(0, ref_loader.REF_ROOT)
    try:
        m = importlib.import_module('backbone_nets.ghostnet_backbone')
    finally:
        sys.path.remove(ref_loader.REF_ROOT)
    return m.ghostnet().eval()


def run_reference(seed, x):
    """dict of everything recorded, from the reference module with the synthetic weights of `seed`."""
    net = reference_module()
    own = net.state_dict()
    sd = synth.make_ghostnet_state(seed)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})      # strict: the key sets are equal
    feats, blocks, gates = {}, {}, {}
    net.act2.register_forward_hook(lambda mod, i, o: feats.__setitem__('pool', o.flatten(1).clone()))
    names = [k for k, *_ in gc.BLOCKS] + ['blocks.9.0']
    for idx, name in enumerate(names):
        mod = net.get_submodule(name)
        mod.register_forward_hook(lambda m_, i, o, idx=idx: blocks.__setitem__(idx, o.clone()))
        if getattr(mod, 'se', None) is not None:
            # the gate is gate_fn(conv_expand output): recompute it from the hooked conv_expand output
            mod.se.conv_expand.register_forward_hook(lambda m_, i, o, idx=idx: gates.__setitem__(idx, (torch.clamp(o + 3.0, 0.0, 6.0) / 6.0).flatten(1)))
    with torch.no_grad():
        out = net(torch.from_numpy(x)).numpy()
    keys = list(own.keys())
    shapes = np.zeros((len(keys), 4), dtype=np.int64)
    ndim = np.zeros(len(keys), dtype=np.int64)
    for i, k in enumerate(keys):
        s = tuple(own[k].shape)
        ndim[i] = len(s)
        shapes[i, :len(s)] = s
    rec = {'out102': out, 'pool': feats['pool'].numpy(), 'keys': np.array(keys), 'shapes': shapes, 'ndim': ndim,
           'block_mean': np.stack([blocks[i].mean(dim=(1, 2, 3)).numpy() for i in range(17)]),
           'block_absmax': np.stack([blocks[i].abs().amax(dim=(1, 2, 3)).numpy() for i in range(17)]),
           'gate_blocks': np.array(sorted(gates)),
           'gate_min': np.stack([gates[i].min(dim=1).values.numpy() for i in sorted(gates)]),
           'gate_max': np.stack([gates[i].max(dim=1).values.numpy() for i in sorted(gates)]),
           'gate_mean': np.stack([gates[i].mean(dim=1).numpy() for i in sorted(gates)]),
           'gate_inside': np.array([float(((gates[i] > 0.05) & (gates[i] < 0.95)).float().mean()) for i in sorted(gates)])}
    return rec


def main():
    torch.manual_seed(0)
    x = synth.normalize_crops(synth.make_crops(2, seed=gc.CROPS_SEED))
    rec = run_reference(gc.SEED, x)
    rec.update({'seed': np.array(gc.SEED), 'crops_seed': np.array(gc.CROPS_SEED)})
    print('out[0,:4] =', rec['out102'][0, :4], 'pool non-zero', float((rec['pool'] != 0).mean()))
    print('block abs-max', rec['block_absmax'].max(axis=1).round(2))
    print('gates inside (0.05, 0.95)', rec['gate_inside'].round(3))
    np.savez_compressed(gc.GOLDEN, **rec)
    print('wrote', gc.GOLDEN, os.path.getsize(gc.GOLDEN), 'bytes')


if __name__ == '__main__':
    main()
