"""ResNeSt-50 without a GPU: the restatement of tests/resnest_cases.py against the recording made from the reference module, the key
table, the flat layout and the FLOP count of the library, the conditions that keep the GPU tests from being vacuous, the two pool
border rules, the constants blob of arch 8, and the refusals that need no device."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resnest_cases as rc          # noqa: E402

N_FLOATS = 25707814
MAC = 1637330432


@pytest.fixture(scope='module')
def golden():
    return np.load(rc.GOLDEN)


@pytest.fixture(scope='module')
def state():
    from synergynet_amd import synth
    return synth.make_resnest50_state(rc.SEED)


@pytest.fixture(scope='module')
def restated(golden, state):
    """(out62, pool, block outputs, attentions) of the restatement in float32 on the golden weights and crops -- computed once."""
    from synergynet_amd import synth
    assert int(golden['seed']) == rc.SEED and int(golden['crops_seed']) == rc.CROPS_SEED
    x = synth.normalize_crops(rc.golden_crops())
    return rc.resnest_forward(state, x, details=True), x


def _compare(got, golden, bar):
    out, pool, blocks, atts = got
    assert out.shape == (2, 62) and pool.shape == (2, 2048) and len(blocks) == 17 and len(atts) == 16
    e_out, e_pool = rc.rel_max(out, golden['out62']), rc.rel_max(pool, golden['pool'])
    mean = np.stack([b.mean(axis=(1, 2, 3)) for b in blocks])
    amax = np.stack([np.abs(b).max(axis=(1, 2, 3)) for b in blocks])
    e_mean, e_max = rc.rel_max(mean, golden['block_mean']), rc.rel_max(amax, golden['block_absmax'])
    e_att = max(rc.rel_max(np.stack([stat(a) for a in atts]), golden[name])
                for name, stat in (('att_min', lambda a: a.min(axis=1)), ('att_max', lambda a: a.max(axis=1)),
                                   ('att_mean', lambda a: a.mean(axis=1))))
    print(f'out62 {e_out:.3g}, pool {e_pool:.3g}, block means {e_mean:.3g}, maxima {e_max:.3g}, attention {e_att:.3g}')
    assert max(e_out, e_pool, e_mean, e_max, e_att) < bar


def test_restatement_matches_the_reference_golden(golden, restated):
    got, _ = restated
    _compare(got, golden, 1e-5)
    for i, a in enumerate(got[3]):
        assert a.shape == (2, 2 * rc.BLOCKS[i][2])
        assert np.abs(a[:, :a.shape[1] // 2] + a[:, a.shape[1] // 2:] - 1.0).max() < 1e-6          # a softmax over the two radix halves


def test_float64_restatement_matches_the_golden(golden, state, restated):
    _, x = restated
    _compare(rc.resnest_forward(state, x, dtype=torch.float64, details=True), golden, 1e-4)


def test_synthetic_checkpoint_exercises_the_network(golden, restated):
    """The conditions that keep the GPU comparisons from being vacuous, on the committed seed."""
    (out, pool, blocks, atts), _ = restated
    for i, b in enumerate(blocks):
        assert 1e-3 < np.abs(b).max() < 16, i
    assert (golden['block_absmax'] < 16).all() and (golden['block_absmax'] > 1e-3).all()
    assert float((pool != 0).mean()) >= 0.4
    for i, a in enumerate(atts):
        assert float(((a > 0.05) & (a < 0.95)).mean()) >= 0.9, i
        assert np.abs(a[0] - a[1]).max() > 1e-2, i
    assert (golden['att_inside'] >= 0.9).all()
    assert np.abs(out[0] - out[1]).max() > 1e-2
    assert np.abs(golden['out62'][0] - golden['out62'][1]).max() > 1e-2


def test_border_rules_bite(state):
    """layer3.0 reads a 15^2 map: the avd pool (3x3 / 2, pad 1) divides by 9 at the borders too, the downsample pool (2x2 / 2, ceil mode)
    by the samples inside.  Either rule swapped for the other's moves the block's output by more than 100 TOL: a port that got one
    wrong cannot hide under the tolerance."""
    block = 1 + [b[0] for b in rc.BLOCKS].index('layer3.0')
    s = rc.block_shapes()[block]
    assert (s['hin'], s['hout'], s['avd']) == (15, 8, True)
    x = np.abs(np.random.default_rng(15).standard_normal((2, 15, 15, s['cin']))).astype(np.float32)      # post-ReLU activations
    right, _ = rc.block_reference(state, block, x)
    for wrong in ({'avd_real_count': True}, {'down_div4': True}):
        e = rc.rel_max(rc.block_reference(state, block, x, **wrong)[0], right)
        print(wrong, f'{e:.3g}')
        assert e > 100 * rc.TOL, wrong


def test_keys_equal_the_reference_state_dict(golden):
    from synergynet_amd import synth
    from synergynet_amd.synergy3DMM import resnest50_keys
    rec = [(str(k), tuple(int(v) for v in s[:n])) for k, s, n in zip(golden['keys'], golden['shapes'], golden['ndim'])]
    assert len(rec) == 482 and sum(k.endswith('num_batches_tracked') for k, _ in rec) == 71
    ours = []
    for k, s in resnest50_keys():                                  # extend by the num_batches_tracked entries, where the module has them
        ours.append((k, s))
        if k.endswith('running_var'):
            ours.append((k[:-len('running_var')] + 'num_batches_tracked', ()))
    assert ours == rec                                             # names, shapes AND the module's order
    assert sum(int(np.prod(s)) for k, s in resnest50_keys()) == N_FLOATS
    sd = synth.make_resnest50_state(1)
    assert set(sd) == {k for k, _ in rec}                          # the synthetic state carries num_batches_tracked as the module does
    assert synth.resnest50_blocks() == rc.BLOCKS
    assert [n for n, _ in synth.RESNEST_HEADS] == ['fc_ori', 'fc_shape', 'fc_exp', 'fc_tex']


def _lib():
    from synergynet_amd import abi
    return abi.lib()


def test_flat_layout_and_flops_match_library():
    from synergynet_amd import synth
    from synergynet_amd.synergy3DMM import ARCH_BY_ID, ARCH_IDS, ARCH_NAMES, flatten_backbone
    assert ARCH_IDS['resnest50'] == rc.ARCH_ID == 8 and 5 not in ARCH_BY_ID and 7 not in ARCH_BY_ID and ARCH_BY_ID[8] == 'resnest50'
    assert {ARCH_BY_ID[i]: i for i in ARCH_BY_ID} == ARCH_IDS
    assert ARCH_NAMES == ('mobilenet_v2', 'resnet50', 'mobilenet_1', 'mobilenet_05', 'mobilenet_2')
    lib = _lib()
    sd = synth.make_resnest50_state(5)
    flat = flatten_backbone(sd, arch='resnest50')
    assert flat.size == lib.syn_resnest50_flat_count() == N_FLOATS
    assert rc.mac_per_face() == MAC
    assert lib.syn_resnest50_flops_per_face() == 2.0 * MAC
    hdr = open(os.path.join(ROOT, 'include', 'synergy_hip.h')).read()
    assert '2 x 1 637 330 432 MAC' in hdr and '25 707 814 floats' in hdr
    # flat is the state_dict order: the first and the last tensors sit where the key table says
    assert np.array_equal(flat[:864], sd['conv1.0.weight'].reshape(-1)) and np.array_equal(flat[-40:], sd['fc_tex.bias'])
    bad = dict(sd); del bad['layer3.0.conv2.fc1.bias']
    with pytest.raises(RuntimeError, match='missing'):
        flatten_backbone(bad, arch='resnest50')
    bad = dict(sd); bad['layer1.1.downsample.1.weight'] = np.zeros((256, 256, 1, 1), np.float32)
    with pytest.raises(RuntimeError, match='unexpected'):
        flatten_backbone(bad, arch='resnest50')
    bad = dict(sd); bad['layer2.0.conv2.conv.weight'] = bad['layer2.0.conv2.conv.weight'][:, :-4]
    with pytest.raises(RuntimeError, match='shape'):
        flatten_backbone(bad, arch='resnest50')
    pre = {'I2P.backbone.' + k: v for k, v in sd.items()}          # the checkpoint prefix
    assert np.array_equal(flatten_backbone(pre, 'I2P.backbone.', arch='resnest50'), flat)


def test_symbols_in_header_ctypes_table_and_library():
    from synergynet_amd import abi
    lib = _lib()
    hdr = open(os.path.join(ROOT, 'include', 'synergy_hip.h')).read()
    declared = set(re.findall(r'\b(syn_[a-z0-9_]+)\s*\(', hdr))
    for s in ('syn_resnest50_flat_count', 'syn_resnest50_flops_per_face', 'syn_load_backbone_resnest50', 'syn_resnest50_block'):
        assert s in declared and s in abi.EXPORTED_SYMBOLS and hasattr(lib, s)
    assert lib.syn_abi_version() == 1
    assert '5: never assigned | 6 ghostnet | 7: never assigned | 8 resnest50' in hdr
    # no device is touched before the arguments are vetted
    flat = np.zeros(8, np.float32)
    assert lib.syn_load_backbone_resnest50(None, flat.ctypes.data_as(ctypes.c_void_p), 8) == abi.SYN_ERR_INVALID
    buf = np.full(8, 7.0, np.float32)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert lib.syn_resnest50_block(None, 17, 0, p, 1, 8, p, 8, None, 0, None) == abi.SYN_ERR_INVALID
    assert b'syn_resnest50_block' in lib.syn_last_error() and np.all(buf == 7.0)


def test_constants_blob_round_trip_and_rejections():
    from synergynet_amd import abi, synth
    from synergynet_amd.dist import check_constants_host, pack_constants_host
    from synergynet_amd.synergy3DMM import parse_constants_header
    lib = _lib()
    pack = synth.make_3dmm(4, n_vert=300)
    blob = pack_constants_host(pack=pack, backbone_state=synth.make_resnest50_state(3), arch='resnest50')
    hdr = check_constants_host(blob)
    assert hdr['has_backbone'] and hdr['has_basis'] and hdr['arch'] == 8 and hdr['total_bytes'] == blob.size
    assert 256 + 4 * (hdr['backbone_floats'] + hdr['basis_floats']) == blob.size
    assert blob.size == lib.syn_pack_constants_host_bytes(8, 1, 300, 68)
    assert parse_constants_header(blob[:256].tobytes())['arch'] == 8
    assert lib.syn_pack_constants_host_bytes(5, 1, 300, 68) == 0                                   # ids 5 and 7 are still unknown
    assert lib.syn_pack_constants_host_bytes(7, 1, 300, 68) == 0
    for unknown in (5, 7, 9):
        bad = blob.copy(); bad[36:40] = np.frombuffer(np.uint32(unknown).tobytes(), np.uint8)
        with pytest.raises(abi.SynergyHipError, match='backbone size'):
            check_constants_host(bad)
        with pytest.raises(ValueError, match='arch'):
            parse_constants_header(bad[:256].tobytes())
    for other in (0, 1, 2, 6):                                                                     # a resnest50 payload labelled otherwise
        bad = blob.copy(); bad[36:40] = np.frombuffer(np.uint32(other).tobytes(), np.uint8)
        with pytest.raises(abi.SynergyHipError, match='backbone size'):
            check_constants_host(bad)
    other = pack_constants_host(pack=pack, backbone_state=synth.make_ghostnet_state(3), arch='ghostnet')
    bad = other.copy(); bad[36:40] = np.frombuffer(np.uint32(8).tobytes(), np.uint8)               # another arch's payload labelled 8
    with pytest.raises(abi.SynergyHipError, match='backbone size'):
        check_constants_host(bad)
    # a flat array of the wrong architecture is refused by the packer
    flat = np.zeros(int(lib.syn_ghostnet_flat_count()), np.float32)
    out = np.empty(blob.size, np.uint8)
    rc_ = lib.syn_pack_constants_host(8, flat.ctypes.data_as(ctypes.c_void_p), flat.size, None, None, None, None, None, None, 0, 0,
                                      out.ctypes.data_as(ctypes.c_void_p), out.size)
    assert rc_ == abi.SYN_ERR_INVALID


@pytest.mark.parametrize('arch', ['resnest101', 'resnest', 'mobilenet_025', 'mobilenet_075'])
def test_unknown_arch_is_refused_before_a_gpu_is_needed(arch):
    from synergynet_amd import SynergyNet
    with pytest.raises(RuntimeError, match=r'Please choose \[mobilenet_v2, resnet50, resnest50, ghostnet, mobilenet_1, mobilenet_05, mobilenet_2\]'):
        SynergyNet(arch=arch, load_constants=False)
