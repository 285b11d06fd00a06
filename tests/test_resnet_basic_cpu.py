"""resnet18 / resnet34 without a GPU: the restatement of tests/resnet_basic_cases.py against the recording made from the reference modules,
the key table, the flat layout and the FLOP count of the library, the conditions that keep the GPU tests from being vacuous, the two
stride-2 alignments, the constants blob of archs 10 / 11, and the refusals that need no device."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resnet_basic_cases as bc          # noqa: E402

N_ENTRIES = {'resnet18': (128, 20), 'resnet34': (224, 36)}      # state_dict() entries, of which num_batches_tracked
# The range every block's abs-max stays in on the committed seed: the builder (synth.make_resnet_basic_state) scales conv2 and bn2 so
# that a residual sum of two O(1) terms stays O(1); an order of magnitude either way is a checkpoint that blows up or dies.
ABSMAX_RANGE = (0.5, 16.0)


@pytest.fixture(scope='module')
def golden():
    return np.load(bc.GOLDEN)


@pytest.fixture(scope='module')
def states():
    from synergynet_amd import synth
    return {a: synth.make_resnet_basic_state(a, bc.SEED) for a in bc.ARCHS}


@pytest.fixture(scope='module')
def restated(golden, states):
    """per arch (out62, pool, block outputs) of the restatement in float32 on the golden weights and crops -- computed once."""
    from synergynet_amd import synth
    assert int(golden['seed']) == bc.SEED and int(golden['crops_seed']) == bc.CROPS_SEED
    x = synth.normalize_crops(bc.golden_crops())
    return {a: bc.resnet_basic_forward(states[a], a, x, details=True) for a in bc.ARCHS}, x


def _compare(arch, got, golden, bar):
    out, pool, blocks = got
    n = len(bc.blocks(arch)) + 1
    assert out.shape == (2, 62) and pool.shape == (2, 512) and len(blocks) == n
    e_out, e_pool = bc.rel_max(out, golden[arch + '_out102'][:, :62]), bc.rel_max(pool, golden[arch + '_pool'])
    mean = np.stack([b.mean(axis=(1, 2, 3)) for b in blocks])
    amax = np.stack([np.abs(b).max(axis=(1, 2, 3)) for b in blocks])
    e_mean, e_max = bc.rel_max(mean, golden[arch + '_block_mean']), bc.rel_max(amax, golden[arch + '_block_absmax'])
    print(f'{arch}: out62 {e_out:.3g}, pool {e_pool:.3g}, block means {e_mean:.3g}, maxima {e_max:.3g}')
    assert max(e_out, e_pool, e_mean, e_max) < bar


@pytest.mark.parametrize('arch', bc.ARCHS)
def test_restatement_matches_the_reference_golden(arch, golden, restated):
    _compare(arch, restated[0][arch], golden, 1e-5)


@pytest.mark.parametrize('arch', bc.ARCHS)
def test_float64_restatement_matches_the_golden(arch, golden, states, restated):
    _compare(arch, bc.resnet_basic_forward(states[arch], arch, restated[1], dtype=torch.float64, details=True), golden, 1e-5)


@pytest.mark.parametrize('arch', bc.ARCHS)
def test_synthetic_checkpoint_exercises_the_network(arch, golden, restated):
    """The conditions that keep the GPU comparisons from being vacuous, on the committed seed: no block blows up or dies over the 8 / 16
    residual adds, the pool is alive, the two faces differ."""
    out, pool, blocks = restated[0][arch]
    lo, hi = ABSMAX_RANGE
    for i, b in enumerate(blocks):
        assert lo < np.abs(b).max(axis=(1, 2, 3)).min() and np.abs(b).max() < hi, i
    amax = golden[arch + '_block_absmax']
    assert (amax > lo).all() and (amax < hi).all()
    assert float((pool != 0).mean()) >= 0.9 and float((golden[arch + '_pool'] != 0).mean()) >= 0.9
    assert np.abs(out[0] - out[1]).max() > 1e-2
    g = golden[arch + '_out102']
    assert np.abs(g[0, :62] - g[1, :62]).max() > 1e-2


def test_stride2_alignments_bite(states):
    """layer3.0 reads a 15^2 map and writes 8^2: conv1's window of output (y, x) is rows 2y - 1 .. 2y + 1 (pad 1) and the downsample reads
    (2y, 2x).  Either moved by one pixel moves the block's output by more than 100 TOL: a port that got one wrong cannot hide under the
    tolerance.  (Measured on resnet18: 0.415 for the taps, 0.884 for the downsample)"""
    arch = 'resnet18'
    block = 1 + [b[0] for b in bc.blocks(arch)].index('layer3.0')
    s = bc.block_shapes(arch)[block]
    assert (s['hin'], s['hout'], s['stride'], s['down']) == (15, 8, 2, True)
    x = np.abs(np.random.default_rng(15).standard_normal((2, 15, 15, s['cin']))).astype(np.float32)      # post-ReLU activations
    right = bc.block_reference(states[arch], arch, block, x)
    assert right.shape == (2, 8, 8, 256)
    for wrong in ({'taps_pad0': True}, {'down_odd': True}):
        e = bc.rel_max(bc.block_reference(states[arch], arch, block, x, **wrong), right)
        print(wrong, f'{e:.3g}')
        assert e > 100 * bc.TOL, wrong


@pytest.mark.parametrize('arch', bc.ARCHS)
def test_keys_equal_the_reference_state_dict(arch, golden):
    from synergynet_amd import synth
    from synergynet_amd.synergy3DMM import resnet_basic_keys
    rec = [(str(k), tuple(int(v) for v in s[:n])) for k, s, n in zip(golden[arch + '_keys'], golden[arch + '_shapes'], golden[arch + '_ndim'])]
    assert (len(rec), sum(k.endswith('num_batches_tracked') for k, _ in rec)) == N_ENTRIES[arch]
    ours = []
    for k, s in resnet_basic_keys(arch):                           # extend by the num_batches_tracked entries, where the module has them
        ours.append((k, s))
        if k.endswith('running_var'):
            ours.append((k[:-len('running_var')] + 'num_batches_tracked', ()))
    assert ours == rec                                             # names, shapes AND the module's order
    assert sum(int(np.prod(s)) for k, s in resnet_basic_keys(arch)) == bc.FLAT_COUNT[arch]
    assert set(synth.make_resnet_basic_state(arch, 1)) == {k for k, _ in rec}
    assert synth.resnet_basic_blocks(arch) == bc.blocks(arch)


def _lib():
    from synergynet_amd import abi
    return abi.lib()


@pytest.mark.parametrize('arch', bc.ARCHS)
def test_flat_layout_and_flops_match_library(arch):
    from synergynet_amd import synth
    from synergynet_amd.synergy3DMM import ARCH_BY_ID, ARCH_IDS, flatten_backbone
    a = bc.ARCH_ID[arch]
    assert ARCH_IDS[arch] == a and ARCH_BY_ID[a] == arch and 9 not in ARCH_BY_ID
    lib = _lib()
    sd = synth.make_resnet_basic_state(arch, 5)
    flat = flatten_backbone(sd, arch=arch)
    assert flat.size == lib.syn_resnet_basic_flat_count(a) == bc.FLAT_COUNT[arch]
    assert bc.mac_per_face(arch) == bc.MAC_FORWARD[arch]
    assert lib.syn_resnet_basic_flops_per_face(a) == 2.0 * bc.MAC_FORWARD[arch]
    assert lib.syn_resnet_basic_flat_count(9) == 0 and lib.syn_resnet_basic_flat_count(1) == 0
    hdr = open(os.path.join(ROOT, 'include', 'synergy_hip.h')).read()
    assert '2 x 553 011 200' in hdr and '2 x 1 129 564 160' in hdr and '11 238 438 floats' in hdr and '21 354 022' in hdr
    # flat is the state_dict order: the first and the last tensors sit where the key table says
    assert np.array_equal(flat[:9408], sd['conv1.weight'].reshape(-1)) and np.array_equal(flat[-10:], sd['fc_exp.bias'])
    bad = dict(sd); del bad['layer3.0.downsample.1.running_mean']
    with pytest.raises(RuntimeError, match='missing'):
        flatten_backbone(bad, arch=arch)
    bad = dict(sd); bad['layer1.0.downsample.0.weight'] = np.zeros((64, 64, 1, 1), np.float32)
    with pytest.raises(RuntimeError, match='unexpected'):
        flatten_backbone(bad, arch=arch)
    bad = dict(sd); bad['layer2.0.conv1.weight'] = bad['layer2.0.conv1.weight'][:, :-4]
    with pytest.raises(RuntimeError, match='shape'):
        flatten_backbone(bad, arch=arch)
    pre = {'I2P.backbone.' + k: v for k, v in sd.items()}          # the checkpoint prefix
    assert np.array_equal(flatten_backbone(pre, 'I2P.backbone.', arch=arch), flat)
    other = 'resnet34' if arch == 'resnet18' else 'resnet18'      # the other depth's checkpoint is not this one's
    with pytest.raises(RuntimeError, match='unexpected|missing'):
        flatten_backbone(synth.make_resnet_basic_state(other, 5), arch=arch)


def test_symbols_in_header_ctypes_table_and_library():
    from synergynet_amd import abi
    lib = _lib()
    hdr = open(os.path.join(ROOT, 'include', 'synergy_hip.h')).read()
    declared = set(re.findall(r'\b(syn_[a-z0-9_]+)\s*\(', hdr))
    for s in ('syn_resnet_basic_flat_count', 'syn_resnet_basic_flops_per_face', 'syn_load_backbone_resnet_basic', 'syn_resnet_basic_block'):
        assert s in declared and s in abi.EXPORTED_SYMBOLS and hasattr(lib, s)
    assert lib.syn_abi_version() == 1
    assert '5: never assigned | 6 ghostnet | 7: never assigned | 8 resnest50' in hdr
    assert '9: never assigned | 10 resnet18 | 11 resnet34' in hdr
    # no device is touched before the arguments are vetted
    flat = np.zeros(8, np.float32)
    assert lib.syn_load_backbone_resnet_basic(None, 10, flat.ctypes.data_as(ctypes.c_void_p), 8) == abi.SYN_ERR_INVALID
    buf = np.full(8, 7.0, np.float32)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert lib.syn_resnet_basic_block(None, 9, 0, p, 1, 8, p, 8, None) == abi.SYN_ERR_INVALID
    assert b'syn_resnet_basic_block' in lib.syn_last_error() and np.all(buf == 7.0)


def test_constants_blob_round_trip_and_rejections():
    from synergynet_amd import abi, synth
    from synergynet_amd.dist import check_constants_host, pack_constants_host
    from synergynet_amd.synergy3DMM import parse_constants_header, resnet_basic_keys
    lib = _lib()
    pack = synth.make_3dmm(4, n_vert=300)
    blobs = {}
    for arch in bc.ARCHS:
        a = bc.ARCH_ID[arch]
        blob = blobs[arch] = pack_constants_host(pack=pack, backbone_state=synth.make_resnet_basic_state(arch, 3), arch=arch)
        hdr = check_constants_host(blob)
        assert hdr['has_backbone'] and hdr['has_basis'] and hdr['arch'] == a and hdr['total_bytes'] == blob.size
        assert 256 + 4 * (hdr['backbone_floats'] + hdr['basis_floats']) == blob.size
        assert blob.size == lib.syn_pack_constants_host_bytes(a, 1, 300, 68)
        assert parse_constants_header(blob[:256].tobytes())['arch'] == a
        # the packer drops fc_tex: the packed backbone is the flat one minus the BN folding (4 -> 2 per channel) and fc_tex, plus two pad rows
        n_bn = sum(int(s[0]) for k, s in resnet_basic_keys(arch) if k.endswith('running_var'))
        assert hdr['backbone_floats'] == bc.FLAT_COUNT[arch] - 2 * n_bn - (102 * 512 + 102) + 64 * 512 + 64
    assert lib.syn_pack_constants_host_bytes(9, 1, 300, 68) == 0                                   # id 9 is still unknown
    blob = blobs['resnet18']
    bad = blob.copy(); bad[36:40] = np.frombuffer(np.uint32(9).tobytes(), np.uint8)
    with pytest.raises(abi.SynergyHipError, match='backbone size'):
        check_constants_host(bad)
    with pytest.raises(ValueError, match='arch'):
        parse_constants_header(bad[:256].tobytes())
    for other in (0, 1, 2, 6, 8, 11):                                                              # a resnet18 payload labelled otherwise
        bad = blob.copy(); bad[36:40] = np.frombuffer(np.uint32(other).tobytes(), np.uint8)
        with pytest.raises(abi.SynergyHipError, match='backbone size'):
            check_constants_host(bad)
    bad = blobs['resnet34'].copy(); bad[36:40] = np.frombuffer(np.uint32(10).tobytes(), np.uint8)   # resnet34's payload labelled 10
    with pytest.raises(abi.SynergyHipError, match='backbone size'):
        check_constants_host(bad)
    # a flat array of the other depth is refused by the packer
    flat = np.zeros(bc.FLAT_COUNT['resnet34'], np.float32)
    out = np.empty(blob.size, np.uint8)
    rc_ = lib.syn_pack_constants_host(10, flat.ctypes.data_as(ctypes.c_void_p), flat.size, None, None, None, None, None, None, 0, 0,
                                      out.ctypes.data_as(ctypes.c_void_p), out.size)
    assert rc_ == abi.SYN_ERR_INVALID


@pytest.mark.parametrize('arch', ['resnet101', 'resnet152', 'resnext50_32x4d', 'wide_resnet50_2', 'resnet'])
def test_deeper_resnets_are_refused_before_a_gpu_is_needed(arch):
    from synergynet_amd import SynergyNet
    with pytest.raises(RuntimeError, match=r'Please choose \[mobilenet_v2, resnet50, resnest50, ghostnet, mobilenet_1, mobilenet_05, mobilenet_2\], resnet18 or resnet34'):
        SynergyNet(arch=arch, load_constants=False)
