"""ResNeSt-50 without a GPU: the restatement of tests/resnest_cases.py against the recording made from the reference module, the key
table, the flat layout and the FLOP count of the library, the conditions that keep the GPU tests from being vacuous, the two pool
border rules, the constants blob of arch 8, the refusals that need no device, and what the block-level probes of
tests/test_gpu_resnest_blocks.py rest on: their conditions, their teeth, the fused tail's grid table and the bound."""
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


# ---- the block-level probes of tests/test_gpu_resnest_blocks.py: their conditions, their teeth, and the bound -------------------------
import exact_probe as ep          # noqa: E402

PROBE_BATCHES = (1, 3, 5)


def _gaussian_case(block, B=3):
    """the input of test_gpu_resnest.py::test_every_block_alone"""
    s = rc.block_shapes()[block]
    return np.random.default_rng(9000 + 100 * block + B).standard_normal((B, s['hin'], s['hin'], s['cin'])).astype(np.float32)


def test_integer_state_is_a_resnest_checkpoint(state):
    from synergynet_amd.synergy3DMM import flatten_backbone
    sd = rc.make_integer_state()
    assert set(sd) == set(state) and all(np.asarray(sd[k]).shape == np.asarray(state[k]).shape for k in sd)
    assert flatten_backbone(sd, arch='resnest50').size == N_FLOATS
    assert all(np.array_equal(v, np.rint(v)) for k, v in sd.items() if not k.endswith('running_var'))
    for i in range(18):
        f = rc.integer_faces(i)
        assert f.shape == (8,) + rc.hook_counts(i)[0] and all(not np.array_equal(f[a], f[b]) for a in range(8) for b in range(a))


def test_the_two_identities_the_probe_rests_on():
    """exp(float32(-104)) is 0 in fp32 (the device's expf has to agree, or the probe fails and says so), and fl(9 k) * fl(1 / 9) == k for
    every integer k the avd pool's sum can hold in the probe (exactness_violations caps it at NINE_RANGE)."""
    assert np.exp(np.float32(-rc.EXP_ZERO)) == 0 and np.exp(np.float32(-rc.EXP_ZERO)).dtype == np.float32
    assert float(torch.exp(torch.tensor(-rc.EXP_ZERO, dtype=torch.float32))) == 0.0
    k = np.arange(rc.NINE_RANGE + 1, dtype=np.int64)
    ninth = np.float32(1) / np.float32(9)
    assert np.array_equal((9 * k).astype(np.float32) * ninth, k.astype(np.float32))
    assert np.array_equal((9 * k).astype(np.float32) * np.float32(0.5) * ninth, k.astype(np.float32) * np.float32(0.5))      # behind a 0.5 gate


@pytest.mark.parametrize('block', range(18))
def test_integer_probe_is_exact_and_not_vacuous(block):
    """exactness_violations is empty on the 8 distinct faces and on every probe batch (a larger batch holds the same 8 faces): every
    stage exact, no constant output, every ReLU map partly clamped without a dead channel, the avd sum inside the range of the 1 / 9
    identity, the odd map's edges distinct, and a gate of exact 0 / 0.5 / 1 whose saturated channels are saturated by more than 100 x the
    bound of z0 - z1 and depend on the face."""
    assert not rc.exactness_violations(block, rc.integer_faces(block))
    for B in PROBE_BATCHES:
        bad = rc.exactness_violations(block, rc.integer_input(block, B))
        assert not bad, (B, bad)
    if 0 < block < rc.TAIL:
        print(f'block {block}: smallest (|z0 - z1| - {rc.EXP_ZERO:g}) / bound = {rc.GATE_MARGIN[block]:.0f}')
        assert rc.GATE_MARGIN[block] > 100
    print({k: f'{v:.3g}' for k, v in rc.MAGNITUDE.items()})


def test_staged_bottleneck_is_the_bottleneck(state):
    for block in (1, 2, 4, 8, 14, 16):
        x = _gaussian_case(block, 2)
        want, att = rc.block_reference(state, block, x)
        got, a = rc.probe_reference(state, block, x, variant='tap')           # the staged path ...
        assert rc.rel_max(got, want) > 1e-6
        xin = torch.from_numpy(x).double().permute(0, 3, 1, 2)
        with torch.no_grad():
            got, a = rc._bottleneck_staged(state, xin, rc.BLOCKS[block - 1], torch.float64)
        # float64 throughout; the gate's layers are a matrix product here and a conv2d there, which sum in different orders
        assert rc.rel_max(got.permute(0, 2, 3, 1).numpy(), want) < 1e-13 and rc.rel_max(a.numpy(), att) < 1e-13
        assert rc.rel_max(rc.probe_reference(state, block, x, att=att)[0], want) < 1e-13      # the attention handed back in reproduces the block
        for flag in ('avd_real_count', 'down_div4'):                                        # the two flags of _bottleneck, staged
            if flag in rc.variants_of(block):
                with torch.no_grad():
                    got, _ = rc._bottleneck_staged(state, xin, rc.BLOCKS[block - 1], torch.float64, variant=flag)
                assert rc.rel_max(got.permute(0, 2, 3, 1).numpy(), rc.block_reference(state, block, x, **{flag: True})[0]) < 1e-13


def test_variants_exist_where_they_should():
    names = [s['key'] for s in rc.block_shapes()]
    avd = [names.index(k) for k in ('layer2.0', 'layer3.0', 'layer4.0')]
    assert rc.variants_of(0) == rc.variants_of(17) == ()
    for v in ('avd_real_count', 'avd_start', 'gap_div_hout'):
        assert [b for b in range(18) if v in rc.variants_of(b)] == avd
    for v in ('down_div4', 'ds_clamped'):
        assert [b for b in range(18) if v in rc.variants_of(b)] == [names.index('layer3.0')]
    for v in set(rc.VARIANTS) - {'avd_real_count', 'avd_start', 'gap_div_hout', 'down_div4', 'ds_clamped'}:
        assert [b for b in range(18) if v in rc.variants_of(b)] == list(range(1, 17))


def test_every_variant_bites(state):
    """Each one-place mistake of resnest_cases.VARIANTS on every block it exists on.  PROBE_VARIANTS change the float64 reference of the
    integer probe at B = 3, so the equality test of the GPU file fails for a kernel that makes one.  BOUND_VARIANTS sit in front of the
    gate, which the probe saturates on purpose.  On the gaussian checkpoint the attention's bound carries the worst case of conv1 and
    conv2 through two dense layers and comes out between 0.02 and 46 for a number in (0, 1): none of the four moves the attention by
    more than 37 x that bound, most by less than 1 x, so the 100 x asked of them cannot be shown there.  It is shown
    on the gate state (resnest_cases.make_gate_state: the probe's exact U in front of an ordinary gate, bound from an exact U): gap_first,
    gap_div_hout and fc1_bias move the attention by more than 100 x its bound on every block.  gap_last_pixel is visible (> 1 x) on every
    block, but 100 x is out of reach of ANY bound that holds for every summation order: one pixel changes the C gaps by 1 / HW of
    themselves, with signs that do not add up in fc1, about sqrt(C) |w| gap / HW, while fc1's C-term dot product may be off by
    (C + 8) u C |w| gap -- a ratio of 2^24 / (HW sqrt(C) (C + 8)) = 32, 48, 62 and 89 for layer1 .. layer4.
    Printed per variant: the smallest max(err / bound) over its blocks on the gaussian block case of test_every_block_alone (attention
    and output under resnest_cases.block_bound), and how many (variant, block) pairs the rel_max < 1e-4 bar of that test lets through."""
    sd_int, sd_gate = ep.reference_state(rc.make_integer_state()), rc.gate_reference_state(rc.make_gate_state())
    smallest, passed_old, pairs, gate = {}, [], 0, {}
    for block in range(1, 17):
        x = rc.integer_input(block, 3)
        right = [t.astype(np.float32) for t in rc.probe_reference(sd_int, block, x)]
        xg = _gaussian_case(block)
        right_g = rc.probe_reference(state, block, xg)
        bounds = rc.block_bound(state, block, xg)
        for v in rc.variants_of(block):
            got_g = rc.probe_reference(state, block, xg, variant=v)
            ratio_att = ep.bound_ratio(got_g[1], right_g[1], bounds[1])
            ratio = max(ratio_att, ep.bound_ratio(got_g[0], right_g[0], bounds[0]))
            smallest[v] = min(smallest.get(v, np.inf), ratio)
            pairs += 1
            if max(rc.rel_max(got_g[0], right_g[0]), rc.rel_max(got_g[1], right_g[1])) < rc.TOL:
                passed_old.append((v, block))
            if v in rc.PROBE_VARIANTS:                                     # (att_face and res_face may hide in noise, whose faces are alike)
                got = [t.astype(np.float32) for t in rc.probe_reference(sd_int, block, x, variant=v)]
                assert not (np.array_equal(got[0], right[0]) and np.array_equal(got[1], right[1])), (block, v)
            else:
                (att, bound), wrong = rc.gate_reference(sd_gate, block, x), rc.gate_reference(sd_gate, block, x, variant=v)[0]
                gate[v] = min(gate.get(v, np.inf), ep.bound_ratio(wrong, att, bound))
                assert ep.bound_ratio(wrong, att, bound) > (1 if v == 'gap_last_pixel' else 100), (block, v)
    print('smallest err / bound of the attention on the gate state: ' + ', '.join(f'{v} {r:.3g}' for v, r in gate.items()))
    print('smallest max(err / bound) on the gaussian checkpoint: ' + ', '.join(f'{v} {r:.3g}' for v, r in smallest.items()))
    print(f'the 1e-4 bar lets {len(passed_old)} of {pairs} (variant, block) pairs through: {passed_old}')
    assert set(smallest) == set(rc.VARIANTS)


def test_gate_state_has_an_ordinary_gate_behind_an_exact_u(state):
    """resnest_cases.make_gate_state: a ResNeSt checkpoint whose convolutions are the integer probe's (so _gate_pair's exact_sums rule
    applies: it asserts integers and pixel sums below 2^24) and whose attention is ordinary: at least half of it inside (0.05, 0.95),
    different between the faces; torch's own fp32 attention stays under the bound from an exact U, or the bound is wrong."""
    from synergynet_amd.synergy3DMM import flatten_backbone
    sd = rc.make_gate_state()
    assert set(sd) == set(state) and flatten_backbone(sd, arch='resnest50').size == N_FLOATS
    ref, worst = rc.gate_reference_state(sd), {}
    for block in range(1, 17):
        for B in (8,) + PROBE_BATCHES:
            x = rc.integer_faces(block) if B == 8 else rc.integer_input(block, B)
            att, bound = rc.gate_reference(ref, block, x)
            if B == 8:
                assert float(((att > 0.05) & (att < 0.95)).mean()) >= 0.5 and all(np.abs(att[i] - att[j]).max() > 0.1 for i in range(8) for j in range(i)), block
        worst[block] = ep.bound_ratio(rc.probe_reference(sd, block, x, dtype=torch.float32)[1], att, bound)
        assert 0 < bound.max() < 0.02, (block, bound.max())
    print('torch fp32 attention, max(err / bound): ' + ', '.join(f'{b} {r:.3g}' for b, r in worst.items()))
    assert 0 < min(worst.values()) and max(worst.values()) < 1


def test_tail_cases_visit_every_grid_of_the_rule():
    """resnest_cases.TAIL_CASES against tail_split, the launcher's rule restated: on layer4.2 every value the rule can return and every
    change point from both sides; on layer3.0 one face and, for the avd tail and for the downsample-pool tail, both sides of the last
    change (to unsplit); on layer1.1 (N = 256: two values) both sides of its one change."""
    names = [s['key'] for s in rc.block_shapes()]
    cases = {k: sorted(B for key, B, _ in rc.TAIL_CASES if key == k) for k in ('layer4.2', 'layer3.0', 'layer1.1')}
    assert sum(len(v) for v in cases.values()) == len(rc.TAIL_CASES) and all(len(d) > 20 for _, _, d in rc.TAIL_CASES)

    def changes(block, tail, upto=2048):
        s = [rc.splits_at(block, B)[tail] for B in range(1, upto + 1)]
        return [B + 1 for B in range(1, upto) if s[B] != s[B - 1]], set(s)             # the first batch of every new value

    b = names.index('layer4.2')
    assert rc.block_tails(b) == [('combine', 16, 512, 2048)]
    at, values = changes(b, 0)
    assert at == [128, 256, 512, 1024] and values == {16, 8, 4, 2, 1}
    assert cases['layer4.2'] == sorted([B for B in at] + [B - 1 for B in at])
    assert {rc.splits_at(b, B)[0] for B in cases['layer4.2']} == values
    b = names.index('layer3.0')
    assert rc.block_tails(b) == [('avd', 64, 256, 1024), ('dspool', 64, 512, 1024)]
    (at_avd, v_avd), (at_ds, v_ds) = changes(b, 0), changes(b, 1)
    assert at_avd[-1] == 512 and at_ds[-1] == 256 and 1 in v_avd and 1 in v_ds
    assert cases['layer3.0'] == [1, 255, 256, 511, 512]
    assert rc.splits_at(b, 1) == (8, 8) and [rc.splits_at(b, B) for B in (255, 256, 511, 512)] == [(4, 2), (2, 1), (2, 1), (1, 1)]
    b = names.index('layer1.1')
    assert rc.block_tails(b) == [('combine', 900, 64, 256)]
    at, values = changes(b, 0)
    assert at == [73] and values == {2, 1} and cases['layer1.1'] == [72, 73]
    # the rule as the launcher has it, read from the source
    src = open(os.path.join(ROOT, 'synergynet_amd', 'csrc', 'resnest_kernels.hip')).read()
    assert 'split < kRsTailGroups && N / (2 * split) >= 128 && N % (256 * split) == 0' in src
    assert 'constexpr int kRsTailGroups = 1024;' in open(os.path.join(ROOT, 'synergynet_amd', 'csrc', 'syn_internal.h')).read()


def test_torch_fp32_stays_under_the_block_bound(state):
    """torch's own fp32 CPU block against the float64 one on the gaussian checkpoint, on both inputs of the GPU test: max(err / bound) per
    block and part has to be below 1, or the bound is wrong -- and above 0, or it judges nothing.  Bottlenecks as on the GPU: the
    attention under its own bound, the output against the float64 tail that uses the fp32 attention."""
    from synergynet_amd import synth
    rng = np.random.default_rng(79)
    prev, worst = synth.normalize_crops(synth.make_crops(2, seed=904)).transpose(0, 2, 3, 1), {}
    for block in range(18):
        chain = np.ascontiguousarray(prev.astype(np.float32))
        for x in (chain, rng.standard_normal(chain.shape).astype(np.float32)):
            got, aux = rc.probe_reference(state, block, x, dtype=torch.float32)
            if x is chain:
                prev = rc.probe_reference(state, block, x)[0]
            for name, r in rc.judge(state, block, x, got, aux):
                worst[block, name] = max(worst.get((block, name), 0.0), r)
    print('torch fp32 max(err / bound): ' + ', '.join(f'{b}:{n} {r:.3g}' for (b, n), r in worst.items()))
    assert max(worst.values()) < 1.0 and min(worst.values()) > 0.0
