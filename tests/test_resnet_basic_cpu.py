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


# ---- the block-level probes of tests/test_gpu_resnet_basic_blocks.py: their conditions, their teeth, and the bound ------------------------
import exact_probe as ep          # noqa: E402

ALL_BLOCKS = [(a, b) for a in bc.ARCHS for b in range(len(bc.block_shapes(a)))]


@pytest.fixture(scope='module')
def int_states():
    return {a: ep.reference_state(bc.make_integer_state(a)) for a in bc.ARCHS}


def test_probe_constants_and_batches():
    """V_STAR makes the fp32 fold's scale gamma itself, V_STAR64 does the same for the float64 reference; a probe batch of any size is made
    of 8 distinct faces and neighbouring slots differ."""
    assert np.float32(ep.V_STAR) + np.float32(1e-5) == np.float32(1) and np.float64(ep.V_STAR64) + np.float64(1e-5) == 1.0
    for B in (1, 3, 5, 127, 1023):
        idx = ep.batch_index(B)
        assert idx.shape == (B,) and idx.min() >= 0 and idx.max() < 8 and (B < 2 or (idx[1:] != idx[:-1]).all())
    assert sorted(ep.batch_index(8)) == list(range(8))
    for arch in bc.ARCHS:
        f = bc.integer_faces(arch, 1)
        assert all(not np.array_equal(f[i], f[j]) for i in range(8) for j in range(i))
        crops = bc.integer_faces(arch, 0)
        assert crops.shape == (8, 3, 120, 120) and np.array_equal(crops * 256, np.rint(crops * 256)) and crops.min() == -255 / 256 and crops.max() == 255 / 256


@pytest.mark.parametrize('arch,block', ALL_BLOCKS)
def test_integer_probe_is_exact_and_not_vacuous(int_states, arch, block):
    """exactness_violations is empty on the 8 distinct faces, of which every probe batch (B = 1, 3 and the GRID_CASES) is made; so it is
    on every batch.  The narrow value sets are in force exactly where the wide ones would not fit."""
    bad = bc.exactness_violations(int_states[arch], arch, block, bc.integer_faces(arch, block))
    assert not bad, bad
    for B in (1, 3):
        assert np.array_equal(bc.integer_input(arch, block, B), bc.integer_faces(arch, block)[ep.batch_index(B)])
        bad = bc.exactness_violations(int_states[arch], arch, block, bc.integer_input(arch, block, B))
        assert not bad, (B, bad)
    sd = bc.make_integer_state(arch)
    if 0 < block < bc.last_block(arch):
        key, cout = bc.block_shapes(arch)[block]['key'], bc.block_shapes(arch)[block]['cout']
        x, w, g = bc.value_sets(cout)
        assert (cout >= 256) == (x == (-1, 0, 1))
        assert set(np.unique(sd[key + '.conv1.weight'])) == set(w) == set(np.unique(sd[key + '.conv2.weight']))
        assert set(np.unique(sd[key + '.bn2.weight'])) <= set(g) and set(np.unique(bc.integer_faces(arch, block))) == set(x)


@pytest.mark.parametrize('arch', bc.ARCHS)
def test_every_variant_changes_the_probe(int_states, arch):
    """Each one-place mistake of resnet_basic_cases.VARIANTS, applied to the float64 reference of the probe at B = 3, changes at least one
    element on every block it exists on -- the equality test of the GPU file fails for a kernel that makes it.  On the gaussian block
    case of test_every_block_alone the same mistakes are printed as rel_max, the figure the 1e-4 bar looks at: a BasicBlock spreads one
    wrong pixel over nine and every channel, so none of them hides under it at block granularity (0.05 at the least)."""
    from synergynet_amd import synth
    gauss = synth.make_resnet_basic_state(arch, bc.SEED)
    for block in range(1, bc.last_block(arch)):
        x = bc.integer_input(arch, block, 3)
        right = bc.block_reference(int_states[arch], arch, block, x)
        s = bc.block_shapes(arch)[block]
        xg = np.random.default_rng(9000 + block).standard_normal((3, s['hin'], s['hin'], s['cin'])).astype(np.float32)
        right_g = bc.block_reference(gauss, arch, block, xg)
        assert set(bc.variants_of(arch, block)) == set(bc.VARIANTS if s['down'] else [v for v in bc.VARIANTS if v not in bc.STRIDED_ONLY])
        line = []
        for v in bc.variants_of(arch, block):
            wrong = bc.block_reference(int_states[arch], arch, block, x, variant=v)
            n = int((wrong.astype(np.float32) != right.astype(np.float32)).sum())
            line.append(f'{v} {n} el, gaussian rel_max {bc.rel_max(bc.block_reference(gauss, arch, block, xg, variant=v), right_g):.3g}')
            assert n > 0, (arch, block, v)
        print(f'{arch} block {block} ({s["key"]}): ' + '; '.join(line))


def test_old_and_new_alignment_variants_are_the_same_mistake(states):
    x = np.random.default_rng(3).standard_normal((2, 15, 15, 128)).astype(np.float32)
    block = 1 + [b[0] for b in bc.blocks('resnet18')].index('layer3.0')
    for v in ('taps_pad0', 'down_odd'):
        assert np.array_equal(bc.block_reference(states['resnet18'], 'resnet18', block, x, variant=v),
                              bc.block_reference(states['resnet18'], 'resnet18', block, x, **{v: True}))


@pytest.mark.parametrize('arch', bc.ARCHS)
def test_torch_fp32_stays_under_the_block_bound(states, arch):
    """torch's own fp32 CPU block against the float64 one on the gaussian checkpoint, both inputs of the GPU test (the previous block's
    output on real crops, and a sign-mixed N(0,1) tensor): max(err / bound) per block has to be below 1, or the bound is wrong."""
    from synergynet_amd import synth
    sd = states[arch]
    rng = np.random.default_rng(78)
    prev = synth.normalize_crops(synth.make_crops(2, seed=902))
    worst = []
    for block in range(len(bc.block_shapes(arch))):
        chain = prev.astype(np.float32)
        ratios = []
        for x in (chain, rng.standard_normal(chain.shape).astype(np.float32)):
            ref, bound = bc.block_reference(sd, arch, block, x), bc.block_bound(sd, arch, block, x)
            ratios.append(ep.bound_ratio(bc.block_reference(sd, arch, block, x, dtype=torch.float32), ref, bound))
            if x is chain:
                prev = ref
        worst.append(max(ratios))
    print(f'{arch} torch fp32 max(err / bound) per block: ' + ', '.join(f'{i}:{r:.3g}' for i, r in enumerate(worst)))
    assert max(worst) < 1.0 and min(worst) > 0.0
