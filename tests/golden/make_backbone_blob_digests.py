"""Generate tests/golden/backbone_blob_digests.npz from THIS project's library, without a device.

    python tests/golden/make_backbone_blob_digests.py

For each of the nine architectures: the backbone-only constants blob of synth.make_*_state(seed 3) as syn_pack_constants_host packs it
(backbone_blob_cases.blob_record): its size, backbone_floats of its header and the sha256 of all its bytes.  And what the device-free
size queries of the C ABI answer for every arch id 0..12 and syn_workspace_bytes for B = 1 and 1024 (backbone_blob_cases.abi_numbers).
The file records what the library computes at the commit that wrote it; regenerate it only with a change that is MEANT to move a packed
backbone (and then bump kConstVersion)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..', '..')))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..')))

import backbone_blob_cases as bc          # noqa: E402


def main():
    rec = {'seed': np.array(bc.SEED), 'archs': np.array(bc.ARCHS), 'arch_ids': np.array(list(bc.ARCH_ID_RANGE)),
           'workspace_batches': np.array(bc.WORKSPACE_BATCHES)}
    size, floats, sha = [], [], []
    for arch in bc.ARCHS:
        s, f, d = bc.blob_record(arch)
        print(f'{arch:14s} {s:12d} bytes  {f:10d} floats  sha256 {d[:16]}')
        size.append(s), floats.append(f), sha.append(d)
    rec.update(blob_bytes=np.array(size, dtype=np.uint64), backbone_floats=np.array(floats, dtype=np.uint64), sha256=np.array(sha))
    rec.update(bc.abi_numbers())
    np.savez_compressed(bc.DIGESTS, **rec)
    print('wrote', bc.DIGESTS, os.path.getsize(bc.DIGESTS), 'bytes')


if __name__ == '__main__':
    main()
