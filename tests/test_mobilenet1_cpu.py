"""CPU-side tests (no GPU) of the MobileNetV1 backbones: the torch restatement the GPU tests compare against is itself held against
the reference module's recorded outputs (tests/golden/mobilenet1_outputs.npz, make_mobilenet1_golden.py), and the host side of the
library -- key tables, flat layout, C symbols, the device-free constants blob -- knows the three architectures."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import mobilenet1_cases as mc


@pytest.fixture(scope='module')
def golden():
    return np.load(mc.GOLDEN)


@pytest.fixture(scope='module')
def golden_crops(golden):
    from synergynet_amd import synth
    return synth.normalize_crops(synth.make_crops(2, seed=int(golden['crops_seed'])))


@pytest.mark.parametrize('width', [1.0, 0.5, 2.0])
def test_restatement_matches_the_reference_golden(golden, golden_crops, width):
    from synergynet_amd import synth
    t = mc.TAG[width]
    sd = synth.make_mobilenet1_state(int(golden[f'seed_{t}']), width)
    out, pool = mc.mobilenet1_forward(sd, golden_crops, width)
    assert out.shape == (2, 102) and pool.shape == (2, int(1024 * width))
    e_out, e_pool = mc.rel_max(out, golden[f'out102_{t}']), mc.rel_max(pool, golden[f'pool_{t}'])
    print(f'width {width}: out102 {e_out:.3g}, pool {e_pool:.3g}')
    assert e_out < mc.TOL and e_pool < mc.TOL
    assert float((golden[f'pool_{t}'] != 0).mean()) > 0.5          # the fixture exercises the network, not a dead ReLU


@pytest.mark.parametrize('width', [1.0, 0.5, 2.0])
def test_restatement_matches_the_live_reference_module(width):
    """On a fresh seed, against the reference's own module where its tree is present (the authoring container)."""
    from oracle import ref_loader
    if not os.path.isfile(os.path.join(ref_loader.REF_ROOT, 'backbone_nets', 'mobilenetv1_backbone.py')):
        pytest.skip('reference tree not present')
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    import make_mobilenet1_golden as mg
    from synergynet_amd import synth
    x = synth.normalize_crops(synth.make_crops(2, seed=977))
    seed = 4242 + int(width * 10)
    want_out, want_pool, _, _, _ = mg.run_reference(width, seed, x)
    out, pool = mc.mobilenet1_forward(synth.make_mobilenet1_state(seed, width), x, width)
    e_out, e_pool = mc.rel_max(out, want_out), mc.rel_max(pool, want_pool)
    print(f'width {width}: out102 {e_out:.3g}, pool {e_pool:.3g}')
    assert e_out < mc.TOL and e_pool < mc.TOL


@pytest.mark.parametrize('width', [1.0, 0.5, 2.0])
def test_keys_equal_the_reference_state_dict(golden, width):
    from synergynet_amd import synth
    from synergynet_amd.synergy3DMM import mobilenet1_keys
    t = mc.TAG[width]
    rec = [(str(k), tuple(int(v) for v in s[:n])) for k, s, n in zip(golden[f'keys_{t}'], golden[f'shapes_{t}'], golden[f'ndim_{t}'])]
    assert any(k.endswith('num_batches_tracked') for k, _ in rec)
    want = [(k, s) for k, s in rec if not k.endswith('num_batches_tracked')]
    ours = mobilenet1_keys(width)
    assert ours == want                                            # names, shapes AND the module's order
    assert {k for k, _ in want} >= {'fc_tex.weight', 'fc_tex.bias'}
    sd = synth.make_mobilenet1_state(1, width)
    assert set(sd) == {k for k, _ in rec}                          # the synthetic state carries num_batches_tracked as the module does


def test_block_table():
    from synergynet_amd import synth
    b = synth.mobilenet1_blocks(1.0)
    assert [k for k, *_ in b] == mc.BLOCKS
    assert b[0] == ('dw2_1', 32, 64, 1) and b[5] == ('dw4_2', 256, 512, 2) and b[-1] == ('dw6', 1024, 1024, 1)
    assert [k for k, _, _, s in b if s == 2] == list(mc.STRIDE2)
    assert synth.mobilenet1_blocks(0.5)[0] == ('dw2_1', 16, 32, 1) and synth.mobilenet1_blocks(2.0)[-1] == ('dw6', 2048, 2048, 1)
    assert synth.MOBILENET1_HEADS == [('fc_ori', 12), ('fc_shape', 40), ('fc_exp', 10), ('fc_tex', 40)]


def _lib():
    from synergynet_amd import abi
    import torch  # noqa: F401
    return abi.lib()


@pytest.mark.parametrize('arch', ['mobilenet_1', 'mobilenet_05', 'mobilenet_2'])
def test_flat_layout_matches_library(arch):
    from synergynet_amd import synth
    from synergynet_amd.synergy3DMM import ARCH_NAMES, flatten_backbone
    w = mc.WIDTHS[arch]
    assert ARCH_NAMES.index(arch) == mc.ARCH_IDS[arch]
    flat = flatten_backbone(synth.make_mobilenet1_state(5, w), arch=arch)
    lib = _lib()
    assert flat.size == lib.syn_mobilenet1_flat_count(mc.ARCH_IDS[arch])
    # the exact count: stem 27 c0 MAC x 60^2, per block (9 cin + cin cout) x hout^2, heads pool x 102
    mac, h = 27 * int(32 * w) * 3600, 60
    for _, cin, cout, s in synth.mobilenet1_blocks(w):
        h = (h - 1) // s + 1
        mac += (9 * cin + cin * cout) * h * h
    assert h == 4
    mac += int(1024 * w) * 102
    assert lib.syn_mobilenet1_flops_per_face(mc.ARCH_IDS[arch]) == 2.0 * mac
    if arch == 'mobilenet_1':
        assert abs(mac / 177e6 - 1) < 0.01                         # "about 177 M MAC per face"
    bad = synth.make_mobilenet1_state(5, w)
    bad['dw4_2.conv_sep.weight'] = bad['dw4_2.conv_sep.weight'][:, :-1]
    with pytest.raises(RuntimeError, match='shape'):
        flatten_backbone(bad, arch=arch)


def test_symbols_in_header_ctypes_table_and_library():
    from synergynet_amd import abi
    lib = _lib()
    hdr = open(os.path.join(ROOT, 'include', 'synergy_hip.h')).read()
    declared = set(re.findall(r'\b(syn_[a-z0-9_]+)\s*\(', hdr))
    for s in ('syn_mobilenet1_flat_count', 'syn_mobilenet1_flops_per_face', 'syn_load_backbone_mobilenet1', 'syn_mobilenet1_layer'):
        assert s in declared and s in abi.EXPORTED_SYMBOLS and hasattr(lib, s)
    assert lib.syn_abi_version() == 1
    for a in (-1, 0, 1, 5):
        assert lib.syn_mobilenet1_flat_count(a) == 0 and lib.syn_mobilenet1_flops_per_face(a) == 0.0
    # no device is touched before the arguments are vetted
    flat = np.zeros(8, np.float32)
    assert lib.syn_load_backbone_mobilenet1(None, 2, flat.ctypes.data_as(ctypes.c_void_p), 8) == abi.SYN_ERR_INVALID
    # ... nor by the per-layer hook: a NULL handle is refused although the (host) pointers would otherwise reach a launch
    buf = np.full(8, 7.0, np.float32)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert lib.syn_mobilenet1_layer(None, 14, 0, p, 0, 1, 8, p, 8, None, 0, None) == abi.SYN_ERR_INVALID
    assert b'syn_mobilenet1_layer' in lib.syn_last_error() and np.all(buf == 7.0)


def test_constants_blob_round_trip_and_rejections():
    from synergynet_amd import abi, synth
    from synergynet_amd.dist import check_constants_host, pack_constants_host
    from synergynet_amd.synergy3DMM import parse_constants_header
    lib = _lib()
    pack = synth.make_3dmm(4, n_vert=300)
    blobs = {}
    for arch, a in mc.ARCH_IDS.items():
        blob = pack_constants_host(pack=pack, backbone_state=synth.make_mobilenet1_state(3, mc.WIDTHS[arch]), arch=arch)
        hdr = check_constants_host(blob)
        assert hdr['has_backbone'] and hdr['has_basis'] and hdr['arch'] == a and hdr['total_bytes'] == blob.size
        assert 256 + 4 * (hdr['backbone_floats'] + hdr['basis_floats']) == blob.size
        assert blob.size == lib.syn_pack_constants_host_bytes(a, 1, 300, 68)
        blobs[arch] = (blob, hdr)
    assert len({h['backbone_floats'] for _, h in blobs.values()}) == 3
    assert lib.syn_pack_constants_host_bytes(5, 1, 300, 68) == 0
    blob, hdr = blobs['mobilenet_1']
    bad = blob.copy(); bad[36:40] = np.frombuffer(np.uint32(5).tobytes(), np.uint8)                  # arch word 5: unknown
    with pytest.raises(abi.SynergyHipError, match='backbone size'):
        check_constants_host(bad)
    with pytest.raises(ValueError, match='arch'):
        parse_constants_header(bad[:256].tobytes())
    for other in ('mobilenet_05', 'mobilenet_2'):                                                   # backbone_floats of another arch
        bad = blob.copy(); bad[40:48] = np.frombuffer(np.uint64(blobs[other][1]['backbone_floats']).tobytes(), np.uint8)
        with pytest.raises(abi.SynergyHipError, match='backbone size'):
            check_constants_host(bad)
    bad = blob.copy(); bad[36:40] = np.frombuffer(np.uint32(0).tobytes(), np.uint8)                  # a mobilenet_1 payload labelled mobilenet_v2
    with pytest.raises(abi.SynergyHipError, match='backbone size'):
        check_constants_host(bad)
    # a flat array of the wrong architecture is refused by the packer
    flat = np.zeros(int(lib.syn_mobilenet1_flat_count(3)), np.float32)
    out = np.empty(blob.size, np.uint8)
    rc = lib.syn_pack_constants_host(2, flat.ctypes.data_as(ctypes.c_void_p), flat.size, None, None, None, None, None, None, 0, 0,
                                     out.ctypes.data_as(ctypes.c_void_p), out.size)
    assert rc == abi.SYN_ERR_INVALID


@pytest.mark.parametrize('arch', ['mobilenet_025', 'mobilenet_075', 'mobilenet_3'])
def test_unsupported_widths_are_refused_before_a_gpu_is_needed(arch):
    from synergynet_amd import SynergyNet
    with pytest.raises(RuntimeError, match=r'Please choose \[.*mobilenet_1, mobilenet_05, mobilenet_2\]'):
        SynergyNet(arch=arch, load_constants=False)


# ---- the integer probe of tests/test_gpu_mobilenet1_layers.py: two conditions on the reference alone ----
def test_probe_running_var_makes_the_scale_gamma():
    """fl32(v* + 1e-5f) == 1.0f, so the library's sqrtf gives 1 and scale == gamma exactly; asserted, not trusted"""
    v = mc.V_STAR
    assert v.dtype == np.float32 and np.float32(v + np.float32(1e-5)) == np.float32(1.0)
    assert np.float32(np.float32(0.5) / np.sqrt(np.float32(v + np.float32(1e-5)))) == np.float32(0.5)
    import torch
    assert mc.V_STAR64 + 1e-5 == 1.0 and float(torch.sqrt(torch.tensor(mc.V_STAR64, dtype=torch.float64) + 1e-5)) == 1.0      # the reference's side
    sd = mc.make_integer_state(mc.PROBE_SEED, 0.5)
    assert all(np.all(a == mc.V_STAR64) and a.dtype == np.float64 for k, a in mc.reference_state(sd).items() if k.endswith('running_var'))
    for k, a in sd.items():
        if k.endswith('running_var'):
            assert a.dtype == np.float32 and np.all(a == v)
        elif k.endswith('running_mean'):
            assert not a.any()
        elif k.endswith('bn_dw.weight') or k.endswith('bn_sep.weight') or k == 'bn1.weight':
            assert set(np.unique(a)) <= {0.5, 1.0, 2.0, -1.0}
        elif k.endswith('.weight'):
            assert set(np.unique(a)) == {-2.0, -1.0, 1.0, 2.0}              # conv and head weights: small integers, no zero
        elif k.endswith('.bias'):
            assert np.all(a == np.rint(a))


@pytest.mark.parametrize('arch', ['mobilenet_1', 'mobilenet_05', 'mobilenet_2'])
def test_probe_is_exact_in_fp32_and_not_hidden_by_relu(arch):
    """For every layer and batch the GPU test uses.  1. Exactness: every stage's largest possible partial sum times the common
    denominator of its terms is below 2^24, and the float64 reference is unchanged by a cast to fp32.  2. ReLU does not hide the
    probe: at most 25 % of a map's elements are 0 and no channel is all 0; at least 1 % are 0, so the clamp itself is exercised
    (pool and heads have no clamp: only the first two apply).  Conditions on the inputs, not tolerances."""
    w = mc.WIDTHS[arch]
    sd = mc.reference_state(mc.make_integer_state(mc.PROBE_SEED, w))
    for layer in range(15):
        for B in mc.probe_batches(w, layer):
            x = mc.integer_input(layer, w, B)
            assert np.all(x == np.rint(x)) and (x.dtype == np.uint8 if layer == 0 else (x.min() == -3 and x.max() == 3))
            assert all(not np.array_equal(x[i], x[i + 1]) for i in range(B - 1))
            ref = mc.layer_reference(sd, w, layer, mc.normalize_u8(x) if layer == 0 else x)
            for name, m in mc.exactness_margin(sd, w, layer, x):
                assert m < 2 ** 24, f'layer {layer} B={B} {name}: {m:.4g}'
            outs = [('out', ref)] if layer == 0 else [('depthwise' if layer < 14 else 'pool', ref[0]), ('out', ref[1])]
            for name, r in outs:
                assert r.dtype == np.float64 and np.array_equal(r.astype(np.float32).astype(np.float64), r)
                zeros = float((r == 0).mean())
                assert zeros <= 0.25, f'layer {layer} B={B} {name}: {zeros:.3f} zeros'
                assert (r != 0).reshape(-1, r.shape[-1]).any(axis=0).all(), f'layer {layer} B={B} {name}: a dead channel'
                if layer < 14:
                    assert zeros >= 0.01, f'layer {layer} B={B} {name}: {zeros:.4f} zeros'


def test_probe_batches_cover_the_tiling_edges():
    for w in (1.0, 0.5, 2.0):
        hout = [s[2] for s in mc.layer_shapes(w)]
        assert hout == [60, 60, 30, 30, 15, 15, 8, 8, 8, 8, 8, 8, 4, 4, 1]
        assert [mc.probe_batches(w, l) for l in (0, 1, 2, 4, 5, 6, 12, 13, 14)] == [[1], [1], [1], [1, 3], [1, 3], [1, 5], [1, 5], [1, 5], [1, 5]]
    from synergynet_amd import synth
    for w in (1.0, 0.5, 2.0):
        assert [(s[1], s[3]) for s in mc.layer_shapes(w)[1:14]] == [(ci, co) for _, ci, co, _ in synth.mobilenet1_blocks(w)]
    assert mc.layer_shapes(0.5)[1][:4] == (60, 16, 60, 32) and mc.layer_shapes(2.0)[13] == (4, 2048, 4, 2048)


def test_layer_references_chain_to_the_whole_network():
    """layer_reference 0..14 fed into each other IS mobilenet1_forward in float64: the same operations, on NHWC-strided tensors, so the
    sums may run in another order -- 1e-12, four decades above float64 rounding and five below anything fp32 can show"""
    import torch
    from synergynet_amd import synth
    w = 0.5
    sd = synth.make_mobilenet1_state(mc.SEEDS[w], w)
    x = synth.normalize_crops(synth.make_crops(2, seed=11))
    want, want_pool = mc.mobilenet1_forward(sd, x, w, torch.float64)
    y = mc.layer_reference(sd, w, 0, x)
    for layer in range(1, 14):
        _, y = mc.layer_reference(sd, w, layer, y)
    pool, out = mc.layer_reference(sd, w, 14, y)
    assert pool.shape == want_pool.shape and out.shape == (2, 62)
    assert mc.rel_max(pool, want_pool) < 1e-12 and mc.rel_max(out, want[:, :62]) < 1e-12


def test_fp32_layers_stay_within_the_derived_bound():
    """torch's own fp32 layers against the float64 reference, judged by layer_bound as the GPU test judges the kernels (real crops,
    B = 1, every layer of mobilenet_05 here; all three widths were measured at 0.26 of the bound at the most)."""
    import torch
    from synergynet_amd import synth
    w = 0.5
    sd = synth.make_mobilenet1_state(mc.SEEDS[w], w)
    prev, worst = synth.normalize_crops(synth.make_crops(1, seed=12)).astype(np.float64), 0.0
    for layer in range(15):
        x = prev.astype(np.float32)
        ref, got, bound = mc.layer_reference(sd, w, layer, x), mc.layer_reference(sd, w, layer, x, torch.float32), mc.layer_bound(sd, w, layer, x)
        if layer == 0:
            pairs = [(got, ref, bound)]
        elif layer < 14:
            pairs = [(got[0], ref[0], bound[0]), (got[1], ref[1], bound[1]),
                     (got[1], mc.pointwise_reference(sd, layer, got[0]), mc.pointwise_bound(sd, layer, got[0]))]
        else:
            pairs = [(got[0], ref[0], bound[0]), (got[1], mc.heads_reference(sd, got[0]), mc.heads_bound(sd, got[0]))]
        for g, r, b in pairs:
            assert g.dtype == np.float32 and b.shape == r.shape == g.shape and float((b > 0).mean()) > 0.7
            worst = max(worst, mc.bound_ratio(g, r, b))
        prev = ref if layer == 0 else ref[1]
    print(f'torch fp32 against float64: max err / bound = {worst:.3f}')
    assert worst < 1.0
