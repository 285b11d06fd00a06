"""GhostNet without a GPU: the restatement of tests/ghostnet_cases.py against the recording made from the reference module, the key
table, the flat layout and the FLOP count of the library, the conditions that keep the GPU tests from being vacuous, the constants
blob of arch 6, and the refusals that need no device."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ghostnet_cases as gc          # noqa: E402


@pytest.fixture(scope='module')
def golden():
    return np.load(gc.GOLDEN)


@pytest.fixture(scope='module')
def restated(golden):
    """(out102, pool, block outputs, gates) of the restatement in float32 on the golden weights and crops -- computed once."""
    from synergynet_amd import synth
    assert int(golden['seed']) == gc.SEED and int(golden['crops_seed']) == gc.CROPS_SEED
    x = synth.normalize_crops(synth.make_crops(2, seed=gc.CROPS_SEED))
    return gc.ghostnet_forward(synth.make_ghostnet_state(gc.SEED), x, details=True), x


def test_restatement_matches_the_reference_golden(golden, restated):
    (out, pool, blocks, gates), _ = restated
    assert out.shape == (2, 102) and pool.shape == (2, 1280) and len(blocks) == 17
    e_out, e_pool = gc.rel_max(out, golden['out102']), gc.rel_max(pool, golden['pool'])
    print(f'out102 {e_out:.3g}, pool {e_pool:.3g}')
    assert e_out < 1e-5 and e_pool < 1e-5
    mean = np.stack([b.mean(axis=(1, 2, 3)) for b in blocks])
    amax = np.stack([np.abs(b).max(axis=(1, 2, 3)) for b in blocks])
    e_mean, e_max = gc.rel_max(mean, golden['block_mean']), gc.rel_max(amax, golden['block_absmax'])
    print(f'block means {e_mean:.3g}, maxima {e_max:.3g}')
    assert e_mean < 1e-4 and e_max < 1e-4
    assert list(golden['gate_blocks']) == gc.SE_BLOCKS == sorted(gates)
    for j, i in enumerate(gc.SE_BLOCKS):
        g = gates[i]
        assert g.shape == (2, gc.BLOCKS[i][2])
        for name, got in (('gate_min', g.min(axis=1)), ('gate_max', g.max(axis=1)), ('gate_mean', g.mean(axis=1))):
            assert gc.rel_max(got, golden[name][j]) < 1e-4, (i, name)


def test_float64_restatement_agrees_with_float32(restated):
    from synergynet_amd import synth
    (out, pool, _, _), x = restated
    o64, p64 = gc.ghostnet_forward(synth.make_ghostnet_state(gc.SEED), x, dtype=torch.float64)
    e_out, e_pool = gc.rel_max(out, o64), gc.rel_max(pool, p64)
    print(f'float32 vs float64: out102 {e_out:.3g}, pool {e_pool:.3g}')
    assert e_out < 1e-4 and e_pool < 1e-4


def test_synthetic_checkpoint_exercises_the_network(golden, restated):
    """The conditions that keep the GPU comparisons from being vacuous, on the committed seed."""
    (out, pool, blocks, gates), _ = restated
    for i, b in enumerate(blocks):
        assert np.abs(b).max() < 16, i
    assert float((pool != 0).mean()) >= 0.4
    for i, g in gates.items():
        assert float(((g > 0.05) & (g < 0.95)).mean()) >= 0.9, i
    assert np.abs(out[0] - out[1]).max() > 1e-2
    assert np.abs(golden['out102'][0] - golden['out102'][1]).max() > 1e-2


def test_keys_equal_the_reference_state_dict(golden):
    from synergynet_amd import synth
    from synergynet_amd.synergy3DMM import ghostnet_keys
    rec = [(str(k), tuple(int(v) for v in s[:n])) for k, s, n in zip(golden['keys'], golden['shapes'], golden['ndim'])]
    assert len(rec) == 518
    ours = []
    for k, s in ghostnet_keys():                                   # extend by the num_batches_tracked entries, where the module has them
        ours.append((k, s))
        if k.endswith('running_var'):
            ours.append((k[:-len('running_var')] + 'num_batches_tracked', ()))
    assert ours == rec                                             # names, shapes AND the module's order
    assert sum(int(np.prod(s)) for k, s in ghostnet_keys()) == 4054138
    sd = synth.make_ghostnet_state(1)
    assert set(sd) == {k for k, _ in rec}                          # the synthetic state carries num_batches_tracked as the module does
    assert [(k, c, m, o, kk, s, se) for k, c, m, o, kk, s, se in synth.ghostnet_blocks()] == gc.BLOCKS


def _lib():
    from synergynet_amd import abi
    return abi.lib()


def test_flat_layout_matches_library():
    from synergynet_amd import synth
    from synergynet_amd.synergy3DMM import ARCH_BY_ID, ARCH_IDS, flatten_backbone
    assert ARCH_IDS['ghostnet'] == gc.ARCH_ID == 6 and 5 not in ARCH_BY_ID and ARCH_BY_ID[6] == 'ghostnet'
    assert {ARCH_BY_ID[i]: i for i in ARCH_BY_ID} == ARCH_IDS
    lib = _lib()
    sd = synth.make_ghostnet_state(5)
    flat = flatten_backbone(sd, arch='ghostnet')
    assert flat.size == lib.syn_ghostnet_flat_count() == 4054138
    mac = gc.mac_per_face()
    assert lib.syn_ghostnet_flops_per_face() == 2.0 * mac == 2.0 * 45802556
    bad = dict(sd); del bad['blocks.3.0.se.conv_reduce.bias']
    with pytest.raises(RuntimeError, match='missing'):
        flatten_backbone(bad, arch='ghostnet')
    bad = dict(sd); bad['blocks.0.0.shortcut.0.weight'] = np.zeros((16, 1, 3, 3), np.float32)
    with pytest.raises(RuntimeError, match='unexpected'):
        flatten_backbone(bad, arch='ghostnet')
    bad = dict(sd); bad['blocks.6.1.ghost2.primary_conv.0.weight'] = bad['blocks.6.1.ghost2.primary_conv.0.weight'][:, :-4]
    with pytest.raises(RuntimeError, match='shape'):
        flatten_backbone(bad, arch='ghostnet')


def test_symbols_in_header_ctypes_table_and_library():
    from synergynet_amd import abi
    lib = _lib()
    hdr = open(os.path.join(ROOT, 'include', 'synergy_hip.h')).read()
    declared = set(re.findall(r'\b(syn_[a-z0-9_]+)\s*\(', hdr))
    for s in ('syn_ghostnet_flat_count', 'syn_ghostnet_flops_per_face', 'syn_load_backbone_ghostnet', 'syn_ghostnet_block'):
        assert s in declared and s in abi.EXPORTED_SYMBOLS and hasattr(lib, s)
    assert lib.syn_abi_version() == 1
    assert '5: never assigned' in hdr
    # no device is touched before the arguments are vetted
    flat = np.zeros(8, np.float32)
    assert lib.syn_load_backbone_ghostnet(None, flat.ctypes.data_as(ctypes.c_void_p), 8) == abi.SYN_ERR_INVALID
    buf = np.full(8, 7.0, np.float32)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert lib.syn_ghostnet_block(None, 17, 0, p, 1, 8, p, 8, None, 0, None) == abi.SYN_ERR_INVALID
    assert b'syn_ghostnet_block' in lib.syn_last_error() and np.all(buf == 7.0)


def test_constants_blob_round_trip_and_rejections():
    from synergynet_amd import abi, synth
    from synergynet_amd.dist import check_constants_host, pack_constants_host
    from synergynet_amd.synergy3DMM import parse_constants_header
    lib = _lib()
    pack = synth.make_3dmm(4, n_vert=300)
    blob = pack_constants_host(pack=pack, backbone_state=synth.make_ghostnet_state(3), arch='ghostnet')
    hdr = check_constants_host(blob)
    assert hdr['has_backbone'] and hdr['has_basis'] and hdr['arch'] == 6 and hdr['total_bytes'] == blob.size
    assert 256 + 4 * (hdr['backbone_floats'] + hdr['basis_floats']) == blob.size
    assert blob.size == lib.syn_pack_constants_host_bytes(6, 1, 300, 68)
    assert parse_constants_header(blob[:256].tobytes())['arch'] == 6
    assert lib.syn_pack_constants_host_bytes(5, 1, 300, 68) == 0                                   # id 5 is still unknown
    assert lib.syn_pack_constants_host_bytes(7, 1, 300, 68) == 0
    bad = blob.copy(); bad[36:40] = np.frombuffer(np.uint32(5).tobytes(), np.uint8)
    with pytest.raises(abi.SynergyHipError, match='backbone size'):
        check_constants_host(bad)
    with pytest.raises(ValueError, match='arch'):
        parse_constants_header(bad[:256].tobytes())
    for other in (0, 1, 2):                                                                        # a ghostnet payload labelled otherwise
        bad = blob.copy(); bad[36:40] = np.frombuffer(np.uint32(other).tobytes(), np.uint8)
        with pytest.raises(abi.SynergyHipError, match='backbone size'):
            check_constants_host(bad)
    other = pack_constants_host(pack=pack, backbone_state=synth.make_mobilenet1_state(3, 1.0), arch='mobilenet_1')
    bad = other.copy(); bad[36:40] = np.frombuffer(np.uint32(6).tobytes(), np.uint8)               # another arch's payload labelled 6
    with pytest.raises(abi.SynergyHipError, match='backbone size'):
        check_constants_host(bad)
    # a flat array of the wrong architecture is refused by the packer
    flat = np.zeros(int(lib.syn_mobilenet1_flat_count(2)), np.float32)
    out = np.empty(blob.size, np.uint8)
    rc = lib.syn_pack_constants_host(6, flat.ctypes.data_as(ctypes.c_void_p), flat.size, None, None, None, None, None, None, 0, 0,
                                     out.ctypes.data_as(ctypes.c_void_p), out.size)
    assert rc == abi.SYN_ERR_INVALID


def test_unknown_arch_is_refused_before_a_gpu_is_needed():
    from synergynet_amd import SynergyNet
    with pytest.raises(RuntimeError, match=r'Please choose \[.*ghostnet, mobilenet_1, mobilenet_05, mobilenet_2\]'):
        SynergyNet(arch='ghostnet_x', load_constants=False)


# ---- the block-level probes of tests/test_gpu_ghostnet_blocks.py: their conditions, their teeth, and the bound -------------------------
import exact_probe as ep          # noqa: E402

PROBE_BATCHES = (1, 3, 5)


def test_integer_state_is_a_ghostnet_checkpoint():
    from synergynet_amd.synergy3DMM import flatten_backbone
    sd = gc.make_integer_state()
    assert flatten_backbone(sd, arch='ghostnet').size == 4054138
    assert all(np.array_equal(v, np.rint(v)) for k, v in sd.items() if k.endswith('.bias') or k.endswith('conv.weight') or k.endswith('.0.weight'))
    for i in range(19):
        f = gc.integer_faces(i)
        assert f.shape == (8,) + gc.hook_counts(i)[0] and all(not np.array_equal(f[a], f[b]) for a in range(8) for b in range(a))


@pytest.mark.parametrize('block', range(19))
def test_integer_probe_is_exact_and_not_vacuous(block):
    """exactness_violations is empty on the 8 distinct faces and on every probe batch (a larger batch holds the same 8 faces): every
    stage exact, no constant output, every ReLU map partly clamped without a dead channel, and on the SE blocks a gate of exact 0 / 1
    that is saturated by more than 100 x the bound of its pre-activation, differs between the faces and is 25 .. 75 % open."""
    assert not gc.exactness_violations(block, gc.integer_faces(block))
    for B in PROBE_BATCHES:
        bad = gc.exactness_violations(block, gc.integer_input(block, B))
        assert not bad, (B, bad)
    if block in gc.SE_BLOCKS:
        print(f'block {block}: smallest (|z| - 3) / bound = {gc.SE_MARGIN[block]:.0f}')
        assert gc.SE_MARGIN[block] > 100


def test_staged_bottleneck_is_the_bottleneck():
    from synergynet_amd import synth
    sd = synth.make_ghostnet_state(gc.SEED)
    for block in (1, 3, 5, 9, 12):
        s = gc.block_shapes()[block]
        x = np.random.default_rng(block).standard_normal((2, s['hin'], s['hin'], s['cin'])).astype(np.float32)
        want, gate = gc.block_reference(sd, block, x)
        xin = torch.from_numpy(x).double().permute(0, 3, 1, 2)
        with torch.no_grad():
            got, g = gc._bottleneck_staged(sd, xin, gc.BLOCKS[block], torch.float64)
        # float64 throughout; the SE convolutions are a matrix product here and a conv2d there, which sum in different orders
        assert gc.rel_max(got.permute(0, 2, 3, 1).numpy(), want) < 1e-13 and (gate is None or gc.rel_max(g.numpy(), gate) < 1e-13)
        if gate is not None:                                          # the gate handed back in reproduces the block
            assert gc.rel_max(gc.probe_reference(sd, block, x, gate=gate)[0], want) < 1e-13


def test_every_variant_changes_the_probe():
    """Each one-place mistake of ghostnet_cases.VARIANTS, applied to the float64 reference of the probe at B = 3, changes at least one
    element on every block it exists on, so the equality test of the GPU file fails for a kernel that makes it.  Printed next to it:
    the rel_max of the same mistake on the gaussian block case of test_every_block_alone, the figure the 1e-4 bar looks at."""
    from synergynet_amd import synth
    sd_int, sd_g = ep.reference_state(gc.make_integer_state()), synth.make_ghostnet_state(gc.SEED)
    seen = set()
    for block in range(16):
        s = gc.block_shapes()[block]
        x = gc.integer_input(block, 3)
        right = gc.probe_reference(sd_int, block, x)[0].astype(np.float32)
        xg = np.random.default_rng(9000 + 100 * block + 3).standard_normal(x.shape).astype(np.float32)
        right_g = gc.probe_reference(sd_g, block, xg)[0]
        line = []
        for v in gc.variants_of(block):
            n = int((gc.probe_reference(sd_int, block, x, variant=v)[0].astype(np.float32) != right).sum())
            line.append(f'{v} {n} el, gaussian rel_max {gc.rel_max(gc.probe_reference(sd_g, block, xg, variant=v)[0], right_g):.3g}')
            assert n > 0, (block, v)
            seen.add(v)
        print(f'block {block} ({s["key"]}): ' + '; '.join(line))
    assert seen == set(gc.VARIANTS)
    assert [b for b in range(18) if 'dw_s2_edge' in gc.variants_of(b)] == [5] and [b for b in range(18) if 'gate_face' in gc.variants_of(b)] == gc.SE_BLOCKS
    assert 'ntail' in gc.variants_of(7) and 'kslot' in gc.variants_of(7) and gc.variants_of(16) == gc.variants_of(17) == ()


def test_torch_fp32_stays_under_the_block_bound():
    """torch's own fp32 CPU block against the float64 one on the gaussian checkpoint, on both inputs of the GPU test: max(err / bound) per
    block and part has to be below 1, or the bound is wrong.  SE blocks as on the GPU: the gate under its own bound, the output against
    the float64 block that uses the fp32 gate."""
    from synergynet_amd import synth
    sd = synth.make_ghostnet_state(gc.SEED)
    rng = np.random.default_rng(79)
    order = [gc.STEM] + list(range(18))
    prev, worst = synth.normalize_crops(synth.make_crops(2, seed=904)), {}
    for block in order:
        chain = prev.astype(np.float32)
        for x in (chain, rng.standard_normal(chain.shape).astype(np.float32)):
            got, aux = gc.probe_reference(sd, block, x, dtype=torch.float32)
            ref, ref_aux = gc.probe_reference(sd, block, x)
            if x is chain:
                prev = ref if block != 17 else None
            for name, r in gc.judge(sd, block, x, got, aux):
                worst[block, name] = max(worst.get((block, name), 0.0), r)
    print('torch fp32 max(err / bound): ' + ', '.join(f'{b}:{n} {r:.3g}' for (b, n), r in worst.items()))
    assert max(worst.values()) < 1.0 and min(worst.values()) > 0.0
