"""CPU-side tests (no GPU) of the ResNet-50 span probes (tests/resnet50_cases.py, tests/test_gpu_resnet50_spans.py): the float64 restatement
is held against the oracle, the integer probe's exactness conditions are asserted per block instead of assumed, the matrix-pipe stem's folded
arithmetic is restated, and the table of launches is held against the thresholds read off the launchers and against the list of kernel
variants the header documents."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import resnet50_cases as rc

TWO_BLOCK = [(1, 2), (3, 4), (4, 5), (7, 8), (16, 17)]


@pytest.fixture(scope='module')
def states():
    sd = rc.make_integer_state()
    return sd, rc.reference_state(sd)


def test_symbol_in_header_ctypes_table_and_library():
    from synergynet_amd import abi
    import torch  # noqa: F401
    lib = abi.lib()
    hdr = open(os.path.join(ROOT, 'include', 'synergy_hip.h')).read()
    assert 'syn_resnet50_span' in set(re.findall(r'\b(syn_[a-z0-9_]+)\s*\(', hdr))
    assert 'syn_resnet50_span' in abi.EXPORTED_SYMBOLS and hasattr(lib, 'syn_resnet50_span')
    assert int(re.search(r'#define SYN_SPAN_AUX_WRITTEN (0x[0-9a-fA-F]+)', hdr).group(1), 16) == 0x10000
    # no device is touched before the arguments are vetted: a NULL handle is refused although the (host) pointers would otherwise reach a launch
    buf = np.full(8, 7.0, np.float32)
    tags = (ctypes.c_int * 160)()
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert lib.syn_resnet50_span(None, 2, 2, p, 0, 1, 8, p, 8, None, 0, tags, 160, None) == abi.SYN_ERR_INVALID
    assert b'syn_resnet50_span' in lib.syn_last_error() and b'expected' in lib.syn_last_error() and np.all(buf == 7.0)


def test_shapes_and_restatement_against_the_oracle():
    """The geometry is the network's; span_reference in fp32 is the oracle (the same torch operations, BatchNorm folded: 1e-5 of the maximum);
    spans fed into each other ARE the whole span in float64 (1e-12)."""
    import torch
    from oracle import resnet_torch
    from synergynet_amd import synth
    shapes = [(b['hin'], b['cin'], b['c'], b['hout'], b['cout'], b['stride'], b['ds'] is not None) for b in rc.BLOCKS]
    assert shapes[0] == (30, 64, 64, 30, 256, 1, True) and shapes[3] == (30, 256, 128, 15, 512, 2, True)
    assert shapes[7] == (15, 512, 256, 8, 1024, 2, True) and shapes[13] == (8, 1024, 512, 4, 2048, 2, True) and shapes[15] == (4, 2048, 512, 4, 2048, 1, False)
    assert [k for k in range(1, 17) if rc.BLOCKS[k - 1]['ds'] is not None] == [1, 4, 8, 14]
    assert rc.span_counts(0, 0, 2) == (2 * 43200, (2, 30, 30, 64), None) and rc.span_counts(17, 17, 2, True) == (2 * 32768, (2, 62), (2, 2048))
    assert rc.span_counts(3, 3, 1, True) == (900 * 256, (1, 30, 30, 256), (1, 30, 30, 128)) and rc.span_counts(16, 16, 1, True)[2] is None
    sd = synth.make_resnet50_state()
    x = synth.normalize_crops(synth.make_crops(2, seed=5))
    want_p, want_pool = resnet_torch.resnet50_forward(sd, x)[:2]
    param, pool = rc.span_reference(sd, 0, 17, x, torch.float32)
    assert rc.bound_ratio(param, want_p.numpy()[:, :62].astype(np.float64), np.full(param.shape, 1e-5 * float(want_p.abs().max()))) < 1
    assert rc.bound_ratio(pool, want_pool.numpy().astype(np.float64), np.full(pool.shape, 1e-5 * float(want_pool.abs().max()))) < 1
    param64, pool64 = rc.span_reference(sd, 0, 17, x)
    y, _ = rc.span_reference(sd, 0, 0, x)
    for first, last in [(1, 1), (2, 7), (8, 8), (9, 16)]:
        y, aux = rc.span_reference(sd, first, last, y)
        if last <= 15:              # the conv1 a fused launch hands over is the next block's own conv1
            t1 = {n: t for n, _, t in rc.span_trace(sd, last + 1, last + 1, y)}[f'{last + 1}.t1']
            assert np.array_equal(aux, rc._nhwc(t1))
    param2, pool2 = rc.span_reference(sd, 17, 17, y)
    assert np.abs(pool2 - pool64).max() <= 1e-12 * np.abs(pool64).max() and np.abs(param2 - param64).max() <= 1e-12 * np.abs(param64).max()


def test_probe_scale_is_the_power_of_two_the_packer_computes(states):
    """The packer folds scale = gamma * (1 / sqrtf(var + 1e-5f)) in fp32 (csrc/synergy_abi.hip pack_backbone_resnet50): with running_var V_STAR
    that is gamma itself, a signed power of two, and with running_mean 0 the shift is the integer bias; asserted, not trusted.  The weights
    are integers, rows differ, no row, input channel or tap is unused, and half of the rows take the pair of big channels with opposite
    weights."""
    import torch
    sd, ref = states
    v = rc.V_STAR
    assert v.dtype == np.float32 and np.float32(v + np.float32(1e-5)) == np.float32(1.0)
    assert float(torch.sqrt(torch.tensor(ref['bn1.running_var'][0], dtype=torch.float64) + 1e-5)) == 1.0
    for ci, c in enumerate(rc.CONVS):
        g, var = sd[c['bn'] + '.weight'], sd[c['bn'] + '.running_var']
        assert g.dtype == var.dtype == np.float32
        scale = (g * (np.float32(1.0) / np.sqrt(var + np.float32(1e-5), dtype=np.float32))).astype(np.float32)
        assert np.array_equal(scale, g) and set(np.unique(np.abs(g))) <= {1.0, 2.0} and (g < 0).any() and (g > 0).any()
        assert not sd[c['bn'] + '.running_mean'].any()
        b, w = sd[c['bn'] + '.bias'], sd[c['key'] + '.weight']
        assert np.array_equal(b, np.rint(b)) and np.array_equal(w, np.rint(w)) and np.abs(w).max() <= 3
        assert w.any(axis=(1, 2, 3)).all() and w.any(axis=(0, 2, 3)).all() and w.any(axis=(0, 1)).all()
        if ci == 0:
            assert w.all() and len(np.unique(np.abs(w))) == 3                # dense, three magnitudes
            continue
        assert len({r.tobytes() for r in w.reshape(w.shape[0], -1)}) == w.shape[0]      # rows differ: swapped K slots change the result
        k1, k2 = rc.BIG(c['cin'])
        pair = w[:, k1] + w[:, k2]                                           # opposite weights in the same tap, or one of the two alone (+1)
        both = (w[:, k1] != 0) & (w[:, k2] != 0)
        assert not pair[both].any() and 0.3 < both.any(axis=(1, 2)).mean() < 0.7
        alone = np.flatnonzero(((w[:, k1] != 0) ^ (w[:, k2] != 0)).any(axis=(1, 2)))
        assert alone.tolist() == ([] if c['role'] == 'ds' else list(rc.BIG(c['cout'])))


@pytest.mark.parametrize('block', range(18))
def test_integer_probe_is_exact_on_every_kernel(states, block):
    """resnet50_cases.exactness_violations on the block's own probe: partial sums below 2^24 in any order, weights x S one fp16 piece (the DUAL
    matrix and the uint8 stem included), every split tensor inside the guard's window, within 22 bits, in two normal pieces, with two channels
    that NEED the low piece -- the fused conv1 of the next block among them.  Each ReLU clamps 30 .. 70 % of its elements on at least a
    quarter of the channels, and no channel is dead on any of the 8 faces."""
    _, ref = states
    assert rc.exactness_violations(ref, block, block, rc.probe_input(block)) == []
    if 1 <= block <= 16:
        shares = rc.relu_shares(ref, block)
        assert set(shares) == {f'{block}.t1', f'{block}.t2', f'{block}.out'}
        for name, (share, dead) in shares.items():
            assert ((share >= 0.3) & (share <= 0.7)).mean() >= 0.25 and not dead, name


@pytest.mark.parametrize('first,last', TWO_BLOCK, ids=[f'{a}-{b}' for a, b in TWO_BLOCK])
def test_integer_probe_stays_exact_through_a_second_block(states, first, last):
    """The two-block spans of the GPU tests start from the first block's probe; the second block then works on the first one's output.  All
    conditions still hold there.  What does not hold any more is the conv1 of a THIRD block, which a fused launch behind the second also
    computes: it outgrows the guard's window, is not returned (no aux is asked for) and is not compared."""
    _, ref = states
    bad = rc.exactness_violations(ref, first, last, rc.probe_input(first))
    assert [b for b in bad if not b.startswith(f'{last + 1}.t1')] == []


def test_matrix_pipe_stem_arithmetic_restated(states):
    """resnet_stem_mfma_kernel takes the raw bytes as fp16 numbers: (2 p - 255) / 256 = p / 128 - 255 / 256 is folded into the filter (w x scale /
    128, one fp16 piece on the probe) and the shift (shift - 255 / 256 sum of w x scale); padding is raw 127.5.  Restated in fp32 with the
    terms added in two different orders, every partial sum is an fp32 number and the result is the float64 reference: the probe's weight set
    (three magnitudes) keeps the stem exact, so it is judged by equality like every other block."""
    import torch
    import torch.nn.functional as F
    sd, ref = states
    w = sd['conv1.weight'].astype(np.float64)
    g, beta = sd['bn1.weight'].astype(np.float64), sd['bn1.bias'].astype(np.float64)
    wf = w * g[:, None, None, None] / 128.0
    shift = beta - 255.0 / 256.0 * (w * g[:, None, None, None]).sum(axis=(1, 2, 3))
    assert np.array_equal(wf.astype(np.float32), wf) and np.array_equal(shift.astype(np.float32), shift)
    S = rc.pow2_scale(np.abs(wf).max())
    hi, lo = rc.f16_pieces(wf * S)
    assert not lo.any() and np.array_equal(hi, wf * S)
    crops = rc.integer_faces(0)[:2]
    raw = torch.from_numpy(crops.astype(np.float32)).permute(0, 3, 1, 2)
    cols = F.unfold(F.pad(raw, (3, 3, 3, 3), value=127.5), 7, stride=2).numpy()                # [2, 147, 3600]: raw bytes, padding 127.5
    terms = cols[:, None, :, :].astype(np.float32) * wf.reshape(1, 64, 147, 1).astype(np.float32)      # fp32 products
    assert np.array_equal(terms.astype(np.float64), cols[:, None].astype(np.float64) * wf.reshape(1, 64, 147, 1))
    fwd = np.cumsum(terms, axis=2, dtype=np.float32)
    rev = np.cumsum(terms[:, :, ::-1], axis=2, dtype=np.float32)
    exact = np.cumsum(terms.astype(np.float64), axis=2)
    assert np.array_equal(fwd.astype(np.float64), exact) and np.array_equal(rev[:, :, -1], fwd[:, :, -1])
    pre = (fwd[:, :, -1] + shift.astype(np.float32)[None, :, None]).reshape(2, 64, 60, 60)
    want = rc.span_trace(ref, 0, 0, rc.probe_input(0)[:2])[0][2]
    got = F.max_pool2d(torch.relu(torch.from_numpy(pre)), 3, 2, 1)
    assert torch.equal(got.double(), want)


def test_pair_layout_restatement():
    """pair_layout against the header comment by hand on one pixel: channel 5 of chunk 1 sits in the high half of dword 32 + 2, its low piece 16
    dwords further"""
    x = np.zeros((1, 64), np.float32)
    x[0, 37] = 2049.0                                   # hi = 2048 (0x6800), lo = 1 (0x3C00)
    d = rc.pair_layout(x)
    assert d[0, 32 + 2] == 0x6800 << 16 and d[0, 32 + 16 + 2] == 0x3C00 << 16 and np.count_nonzero(d) == 2


def test_thresholds_read_off_the_launchers():
    """The batch sizes at which a launcher picks another kernel, as expected_tags derives them from the launchers' conditions:
      * LDS-tiled GEMMs from M >= 4096: B >= 5 / 19 / 64 / 256 in layers 1 / 2 / 3 / 4 (layer 1 only with SYNERGY_HIP_RESNET_FUSE=0: conv3 and
        the downsample branch; under the default fusion its 64-channel conv1 stays on conv_h2s_kernel and the rest is one launch);
      * 256-pixel tiles where steps > 16 and ceil(M / 256) (N / 128) >= 256: layer2 conv2 from 291 (a launch of its own only without the
        fusion), layer3 conv1 / conv2 from 509, layer4.0 conv1 from 253, layer4 conv1 / conv2 from 1009;
      * DUAL from 125 (layer3.0) and 241 (layer4.0); conv_h2s_kernel<2,4,2> from 2048 tiles: layer 1's conv1 from 292;
      * the matrix-pipe stem from 128 uint8 crops; SYNERGY_HIP_RESNET_GEMM=2 puts the 128-pixel tiles on every shape."""
    th = rc.thresholds
    assert th(0, 'default') == [128] and th(0, 'default', in_u8=False) == [] and th(0, 'fp32') == []
    assert th(1, 'default') == th(2, 'default') == th(3, 'default') == [292]
    assert th(1, 'nofuse') == [5, 292] and th(5, 'default') == [19] and th(5, 'nofuse') == [19, 291]
    assert th(8, 'default') == [19, 64, 125, 509] and th(9, 'default') == [64, 509]
    assert th(14, 'default') == [64, 241, 253, 256, 1009] and th(15, 'default') == th(16, 'default') == [256, 1009]
    assert th(17, 'default') == []
    assert all(th(k, 'gemm2') == [] for k in range(4, 17))
    lt = lambda tags: [t % 1000 for t in tags]
    assert lt(rc.expected_tags(9, 9, 63)[0]) == [31, 31, 31] and lt(rc.expected_tags(9, 9, 64)[0]) == [50, 51, 40]
    assert lt(rc.expected_tags(9, 9, 509)[0]) == [52, 53, 40] and lt(rc.expected_tags(9, 9, 3, gemm=2)[0]) == [50, 51, 40]
    assert lt(rc.expected_tags(8, 8, 124)[0]) == [40, 51, 40, 40] and lt(rc.expected_tags(8, 8, 125)[0]) == [40, 51, 60]
    assert lt(rc.expected_tags(1, 2, 3)[0]) == [31, 106, 103] and lt(rc.expected_tags(4, 5, 21)[0]) == [40, 40, 122, 123]
    assert lt(rc.expected_tags(1, 1, 3, fuse=1)[0]) == [31, 31, 104] and lt(rc.expected_tags(1, 1, 3, fuse=0)[0]) == [31, 31, 31, 31]
    assert lt(rc.expected_tags(0, 0, 128)[0]) == [4] and lt(rc.expected_tags(0, 0, 128, fuse=0)[0]) == [3, 5] and lt(rc.expected_tags(0, 0, 127)[0]) == [1, 5]
    assert lt(rc.expected_tags(2, 2, 2331)[0]) == [22, 103]


# which test of tests/test_gpu_resnet50_spans.py asserts a tag list with the code, for every code of include/synergy_hip.h
def _asserted_codes():
    seen = {}
    for sched in rc.SCHEDULES:
        fusion, fuse, gemm = rc.schedule_args(sched)
        for k in range(18):
            for B in rc.probe_batches(k, sched):
                for t in rc.expected_tags(k, k, B, fusion, fuse, gemm)[0]:
                    seen.setdefault(t % 1000, f'{sched} block {k} B={B}')
    for first, last in TWO_BLOCK:
        for t in rc.expected_tags(first, last, 21)[0]:
            seen.setdefault(t % 1000, f'default blocks {first}-{last} B=21')
    for t in rc.expected_tags(2, 2, 2331)[0]:
        seen.setdefault(t % 1000, 'default block 2 B=2331')
    for knobs in ({'lt_glds': 0}, {'lt_glds': 2}, {'lt_stage': 0}, {'lt_stage': 1}):
        for block, batches in [(7, (293, 21)), (8, (511, 125)), (9, (511, 65)), (15, (1011, 257))]:
            for B in batches:
                for t in rc.expected_tags(block, block, B, **knobs)[0]:
                    seen.setdefault(t % 1000, f'{knobs} block {block} B={B}')
    return seen


# conv_f16x2_kernel<1,4>: an input of 2 GiB and fewer than 1024 tiles of 128 pixels x 64 channels exclude each other for every ResNet-50 shape
# (2 GiB of input are at least 2^18 pixels of at most 2048 channels = 2048 tiles of 128).  conv_c3f_kernel of layer 1 (shapes 0 and 1) with an
# fp32 identity, with or without conv2 in front: the only bottleneck whose downsample branch is a launch of its own in front of a fused
# launch is layer2.0, shape 2; the instantiations exist, the network never selects them.
UNREACHED = {21, 100, 102, 110, 112}


def test_every_documented_kernel_variant_is_in_an_asserted_tag_list():
    hdr = open(os.path.join(ROOT, 'include', 'synergy_hip.h')).read()
    doc = hdr[hdr.index('launch_tags[i] = 1000 x block'):hdr.index('#define SYN_SPAN_AUX_WRITTEN')]
    for word in ('resnet_stem_kernel', 'resnet_stem_mfma_kernel', 'maxpool3x3s2_kernel', 'conv_kernel', 'conv_f16x2_kernel', 'conv_h2s_kernel',
                 'conv_lt_kernel', 'conv_lp_kernel', 'DUAL', 'conv_c3f_kernel', 'pool_fc_generic_kernel'):
        assert word in doc, word
    every = {1, 3, 4, 5, 60, 90} | {10 + m for m in (1, 2, 4)} | {20 + m for m in (1, 2)} | {30 + m for m in (1, 2)} | \
        {b + v for b in (40, 50) for v in range(4)} | {100 + 10 * s + 2 * c + r for s in range(3) for c in (0, 1) for r in (0, 1)} | {104, 106}
    seen = _asserted_codes()
    assert set(seen) <= every, set(seen) - every
    assert every - set(seen) == UNREACHED, (sorted(every - set(seen)), sorted(UNREACHED))


@pytest.fixture(scope='module')
def gaussian():
    from synergynet_amd import synth
    sd = synth.make_resnet50_state()
    return sd, rc.gaussian_inputs(sd)


@pytest.mark.parametrize('block', [0, 1, 4, 8, 16, 17])
def test_torch_fp32_stays_under_the_fp32_bound(gaussian, block):
    """torch's own fp32 layers on the gaussian checkpoint against the float64 reference: under the fp32 handle's bound, and the fp16 x2
    handle's bound is the wider one everywhere (it adds terms, it drops none)"""
    import torch
    sd, xs = gaussian
    x = rc.normalize_u8(xs[0]) if block == 0 else xs[block]
    ref, got = rc.span_reference(sd, block, block, x), rc.span_reference(sd, block, block, x, torch.float32)
    b32, b16 = rc.span_bound(sd, block, block, x, fusion=1), rc.span_bound(sd, block, block, x, fusion=2, B=512)
    for i in (0, 1):
        if b32[i] is None:
            continue
        assert rc.bound_ratio(got[i], ref[i], b32[i]) < 1 and (b16[i] >= b32[i]).all() and np.isfinite(b16[i]).all()
    if block == 17:
        assert rc.bound_ratio(got[0], rc.heads_reference(sd, got[1]).numpy(), rc.heads_bound(sd, got[1])) < 1


# by how much the wrong variant leaves the fp16 x2 bound on the gaussian checkpoint, at least (the measured factors are far larger)
FACTOR = 8.0


@pytest.mark.parametrize('kind', list(rc.VARIANTS))
def test_wrong_variants_are_caught_by_both_probes(states, gaussian, kind):
    """Seven mistakes restated in numpy (resnet50_cases.VARIANTS).  Each makes the integer probe DIFFER from the reference, and six of them
    leave the elementwise fp16 x2 bound on the gaussian checkpoint by more than FACTOR (11 x for the stride of the downsample branch, 30 x for
    the padding tap, 93 x for the swapped channels, 339 x for the tail, more for the other two).  The seventh, the dropped lo x hi term, does
    NOT: a missing low piece is 2^-11 of each of conv1's n = 256 terms with mixed signs, about 2^-11 / sqrt(n) = 2^-15 of the magnitude, while
    the bound has to allow 3 n u = 2^-14.4 of it for the summation alone -- the variant stays at 0.04 of the bound, asserted below.  That is
    the case the integer probe's pair channels are there for: there the same mistake is an error of +-1 in an exact result."""
    _, ref = states
    sd, xs = gaussian
    k = rc.VARIANTS[kind]
    want = rc.span_reference(ref, k, k, rc.probe_input(k))[0]
    wrong = rc.variant_output(ref, kind, rc.probe_input(k))
    assert wrong.shape == want.shape and not np.array_equal(wrong, want, equal_nan=True)
    x = rc.normalize_u8(xs[0]) if k == 0 else xs[k]
    B = 512                                              # (the DUAL GEMM and the matrix-pipe stem: the widest bound of the block)
    want, bound = rc.span_reference(sd, k, k, x)[0], rc.span_bound(sd, k, k, x, B=B)[0]
    wrong = rc.variant_output(sd, kind, x)
    with np.errstate(invalid='ignore'):
        ratio = np.nan_to_num(np.abs(wrong - want) / bound, nan=np.inf)
    if kind == 'lohi':
        assert ratio.max() < 1.0, ratio.max()            # (only the integer probe sees it)
    else:
        assert ratio.max() > FACTOR, (kind, ratio.max())
