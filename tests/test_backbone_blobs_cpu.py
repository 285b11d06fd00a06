"""The packed backbones and the device-free size queries, against tests/golden/backbone_blob_digests.npz (written by
tests/golden/make_backbone_blob_digests.py from this project's own library): every architecture packs to the same bytes, and every
count the C ABI answers without a device is the number it was.  No GPU."""
import numpy as np
import pytest

import backbone_blob_cases as bc


@pytest.fixture(scope='module')
def want():
    g = dict(np.load(bc.DIGESTS, allow_pickle=False))
    assert int(g['seed']) == bc.SEED and tuple(g['archs']) == bc.ARCHS
    assert list(g['arch_ids']) == list(bc.ARCH_ID_RANGE) and tuple(g['workspace_batches']) == bc.WORKSPACE_BATCHES
    return g


@pytest.mark.parametrize('arch', bc.ARCHS)
def test_packed_backbone_is_byte_for_byte_the_recorded_one(want, arch):
    i = bc.ARCHS.index(arch)
    size, floats, sha = bc.blob_record(arch)
    print(arch, size, floats, sha)
    assert size == int(want['blob_bytes'][i])
    assert floats == int(want['backbone_floats'][i])
    assert size == 256 + 4 * floats
    assert sha == str(want['sha256'][i])


def test_size_queries_answer_what_they_did(want):
    got = bc.abi_numbers()
    for name, val in got.items():
        print(name, val)
        assert val.dtype == want[name].dtype and np.array_equal(val, want[name]), name
    # one activation workspace serves every backbone: 1 152 000 floats per face, whatever the handle runs
    ws = got['workspace_bytes'].astype(np.int64)
    assert (ws[1] - ws[0]) % (bc.WORKSPACE_BATCHES[1] - bc.WORKSPACE_BATCHES[0]) == 0
    assert (ws[1] - ws[0]) // (bc.WORKSPACE_BATCHES[1] - bc.WORKSPACE_BATCHES[0]) >= 4 * 1152000
    # the ids nobody was ever given pack nothing and count nothing
    for a in (5, 7, 9, 12):
        assert got['host_bytes_backbone'][a] == 0 and got['host_bytes_empty'][a] == 0 and got['host_bytes_both'][a] == 0
        assert got['mobilenet1_flat_count'][a] == 0 and got['resnet_basic_flat_count'][a] == 0
        assert got['mobilenet1_flops_per_face'][a] == 0 and got['resnet_basic_flops_per_face'][a] == 0
