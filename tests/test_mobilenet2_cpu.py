"""CPU-side tests (no GPU) of the MobileNetV2 span probes (tests/mobilenet2_cases.py, tests/test_gpu_mobilenet2_spans.py): the float64
restatement is held against the oracle, the integer probe's exactness conditions are asserted per span instead of assumed, torch's own fp32
layers stay under the derived bound, six wrong variants of a block are caught by both probes (and what the end-of-network tolerance would
have made of them is measured), and the batch lists reach every launch code and both sides of every threshold of the schedule table."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import mobilenet2_cases as mc

SINGLE = [(f, f) for f in range(2, 18)]
PROBED = [(0, 1)] + SINGLE + mc.SPANS


def test_symbol_in_header_ctypes_table_and_library():
    from synergynet_amd import abi
    import torch  # noqa: F401
    lib = abi.lib()
    hdr = open(os.path.join(ROOT, 'include', 'synergy_hip.h')).read()
    assert 'syn_mobilenet2_span' in set(re.findall(r'\b(syn_[a-z0-9_]+)\s*\(', hdr))
    assert 'syn_mobilenet2_span' in abi.EXPORTED_SYMBOLS and hasattr(lib, 'syn_mobilenet2_span')
    # no device is touched before the arguments are vetted: a NULL handle is refused although the (host) pointers would otherwise reach a launch
    buf = np.full(8, 7.0, np.float32)
    tags = (ctypes.c_int * 64)()
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert lib.syn_mobilenet2_span(None, 2, 2, p, 0, 1, 8, p, 8, None, 0, tags, 64, None) == abi.SYN_ERR_INVALID
    assert b'syn_mobilenet2_span' in lib.syn_last_error() and b'expected' in lib.syn_last_error() and np.all(buf == 7.0)


def test_shapes_and_restatement_against_the_oracle():
    """SHAPES is the network's geometry; span_reference in fp32 is the oracle (the same torch operations, BatchNorm folded: 1e-5 of the
    maximum); spans fed into each other ARE the whole span in float64 (other strides, so sums may run in another order: 1e-12)."""
    import torch
    from oracle import backbone_torch
    from synergynet_amd import synth
    assert [mc.SHAPES[f] for f in (0, 1, 2, 4, 7, 14, 17, 18)] == [(120, 3, 60, 32), (60, 32, 60, 16), (60, 16, 30, 24), (30, 24, 15, 32),
                                                                    (15, 32, 8, 64), (8, 96, 4, 160), (4, 160, 4, 320), (4, 320, 4, 1280)]
    assert mc.RESIDUAL == {3, 5, 6, 8, 9, 10, 12, 13, 15, 16} and mc.STRIDE2 == {2, 4, 7, 14}
    sd = synth.make_backbone_state(1234)
    x = synth.normalize_crops(synth.make_crops(2, seed=5))
    want_p, want_pool = backbone_torch.mobilenet_v2_forward(sd, x)
    pool, param = mc.span_reference(sd, 0, 19, x, torch.float32)
    assert mc.rel_max(param, want_p.numpy()) < 1e-5 and mc.rel_max(pool, want_pool.numpy()) < 1e-5
    pool64, param64 = mc.span_reference(sd, 0, 19, x)
    y = mc.span_reference(sd, 0, 1, x)
    for first, last in [(2, 2), (3, 4), (5, 6), (7, 14), (15, 17)]:
        y = mc.span_reference(sd, first, last, y)
    pool2, param2 = mc.span_reference(sd, 18, 19, y)
    assert mc.rel_max(pool2, pool64) < 1e-12 and mc.rel_max(param2, param64) < 1e-12


def test_probe_scale_is_the_power_of_two_the_packer_computes():
    """The packer folds scale = gamma * (1 / sqrtf(var + 1e-5f)) in fp32 (csrc/synergy_abi.hip pack_backbone_mbv2): with running_var V_STAR
    that is gamma itself, a power of two, and with running_mean 0 the shift is the integer bias; asserted, not trusted."""
    import torch
    v = mc.V_STAR
    assert v.dtype == np.float32 and np.float32(v + np.float32(1e-5)) == np.float32(1.0)
    assert mc.V_STAR64 + 1e-5 == 1.0 and float(torch.sqrt(torch.tensor(mc.V_STAR64, dtype=torch.float64) + 1e-5)) == 1.0
    sd = mc.make_integer_state()
    for L in mc.LAYERS:
        g, var = sd[L['bn'] + '.weight'], sd[L['bn'] + '.running_var']
        assert g.dtype == var.dtype == np.float32
        scale = (g * (np.float32(1.0) / np.sqrt(var + np.float32(1e-5), dtype=np.float32))).astype(np.float32)
        assert np.array_equal(scale, g) and set(np.unique(np.abs(g))) <= {1.0, 2.0}
        assert not sd[L['bn'] + '.running_mean'].any()
        b, w = sd[L['bn'] + '.bias'], sd[L['key'] + '.weight']
        assert np.array_equal(b, np.rint(b)) and np.array_equal(w, np.rint(w)) and np.abs(w).max() <= 3
        if L['relu6'] and L['feature'] <= 17:                   # what keeps relu6(x) / 6 a short binary fraction (make_integer_state)
            assert np.array_equal(b / 3, np.rint(b / 3)) and (L['kind'] == 'dw' or set(np.unique(np.abs(w))) <= {0.0, 3.0})
        w2 = w.reshape(w.shape[0], -1)
        assert w2.any(axis=1).all() and (L['kind'] == 'dw' or w2.any(axis=0).all())        # no dead row, no input channel unused
        if L['kind'] in ('stem', 'dw') or L['feature'] == 1:
            assert w.all()                                                                  # dense: no zero tap
        assert len({r.tobytes() for r in w2}) > 0.9 * len(w2) or L['kind'] == 'dw'          # rows differ: swapped k slots change the result
    b1 = sd[mc.feature_layers(1)[-1]['bn'] + '.bias']
    assert np.array_equal(b1 / 3, np.rint(b1 / 3))                  # stem_rm.hip divides features.1's project shift by 6 as well
    ref = mc.reference_state(sd)
    assert all(a.dtype == np.float64 and np.all(a == mc.V_STAR64) for k, a in ref.items() if k.endswith('running_var'))


def test_multiples_of_three_survive_the_division_by_six():
    """The kernels that carry relu6(x) / 6 multiply by the fp32 number nearest to 1 / 6 (times a power of two).  fl(1 / 6) = (1 / 6)(1 + 2^-25),
    so (3 k 2^-q) fl(1 / 6) lies (k 2^-q / 2) 2^-25 above k 2^-q / 2, less than half an ulp of it, and rounds to it: every hidden value
    the probe produces (pre-activations up to 3 x 2^12, q = 0 and q = 8) and every shift comes out of the multiplication exact."""
    sixth = np.float32(1.0) / np.float32(6.0)
    assert abs(float(sixth) * 6.0 - 1.0 - 2.0 ** -25) < 2.0 ** -45
    k = np.arange(-4096, 4097, dtype=np.float64)
    for q in (0, 8):
        x = (3.0 * k * 2.0 ** -q).astype(np.float32)
        assert np.array_equal((x * sixth).astype(np.float64), k * 2.0 ** -q / 2.0)
        for S in (2.0 ** 9, 2.0 ** 12):                              # the scaled accumulator times 1 / (6 S), and times 1 / (96 S) at input scale 16
            assert np.array_equal(((x * np.float32(S)) * (np.float32(1.0) / np.float32(6.0 * S))).astype(np.float64), k * 2.0 ** -q / 2.0)
            assert np.array_equal(((x * np.float32(16 * S)) * (np.float32(1.0) / np.float32(96.0 * S))).astype(np.float64), k * 2.0 ** -q / 2.0)


def test_probe_stays_on_the_fp16_schedule():
    """The load-time range verdict takes a block whose bound leaves the fp16 window off the fp16 x2 kernels: the probe would then judge the
    fallback.  No block of the integer checkpoint (nor of the gaussian one) is flagged at input scale 1 or 16."""
    from synergynet_amd import synth
    for sd in (mc.make_integer_state(), synth.make_backbone_state(1234)):
        u1, u16, bound = mc.range_verdict(sd)
        assert u1 == 0 and u16 == 0
        assert all(1.0 < bound[f] < 3750.0 for f in range(2, 19)), bound


@pytest.mark.parametrize('first,last', PROBED, ids=lambda v: str(v))
def test_probe_exactness_conditions_hold(first, last):
    """mobilenet2_cases.exactness_violations on the eight faces every probe batch is made of: multiples of 2^-q, partial sums below 2^24,
    one-piece weights, two-piece activations at both input scales, no constant output, hidden activations at 0, inside and at 6.  The
    float64 reference survives the cast to fp32, and neighbouring batch slots hold different faces."""
    sd = mc.reference_state(mc.make_integer_state())
    faces = mc.integer_faces(first)
    x = mc.normalize_u8(faces) if first == 0 else faces
    assert faces.dtype == (np.uint8 if first == 0 else np.float32) and np.array_equal(faces, np.rint(faces))
    if first:                                                  # small integers, and the pair channels with their 12-bit values
        k1, k2 = mc.pair_channels(faces.shape[-1])
        small = np.delete(faces, [k1, k2], axis=-1)
        assert small.min() == -4 and small.max() == 4
        assert 2048 < faces[..., [k1, k2]].min() and faces[..., [k1, k2]].max() * 16 <= 65504 and np.abs(faces[..., k1] - faces[..., k2]).max() <= 8
        assert (faces[..., k1] % 2 == 1).any() and (faces[..., k1] % 2 == 0).any()
    assert len({f.tobytes() for f in faces}) == mc.N_FACES
    assert mc.exactness_violations(sd, first, last, x) == []
    ref = mc.span_reference(sd, first, last, x)
    for r in (ref if last == 19 else (ref,)):
        assert r.dtype == np.float64 and np.array_equal(r.astype(np.float32).astype(np.float64), r)
    idx = mc.batch_index(9)
    assert list(idx) == [3, 0, 5, 2, 7, 4, 1, 6, 3] and all(idx[i] != idx[i + 1] for i in range(8))


def test_fp32_layers_stay_within_the_derived_bound():
    """torch's own fp32 layers against the float64 reference on the same fp32 input (real crops handed on block by block, B = 1), judged
    by span_bound('fp32') as the GPU test judges the kernels: every single block, the spans, and the pool.  Measured: 0.009 of the bound
    at the most (features.2; the stem + features.1 0.007, the tails 0.002) -- a fused block returns no hidden tensor, so the bound is
    carried through sum |w| twice inside a block, which real rounding errors do not follow (MobileNetV1's per-layer bound sat at 0.26)."""
    import torch
    from synergynet_amd import synth
    sd = synth.make_backbone_state(1234)
    crops = synth.normalize_crops(synth.make_crops(1, seed=12))
    worst = {}
    for first, last in PROBED:
        x = crops if first == 0 else mc.span_reference(sd, 0, first - 1, crops).astype(np.float32)
        ref, got, bound = mc.span_reference(sd, first, last, x), mc.span_reference(sd, first, last, x, torch.float32), mc.span_bound(sd, first, last, x, 'fp32')
        if last == 19:
            pairs = [(got[0], ref[0], bound[0]), (got[1], mc.heads_reference(sd, got[0]), mc.heads_bound(sd, got[0]))]
        else:
            pairs = [(got, ref, bound)]
        for g, r, b in pairs:
            assert g.dtype == np.float32 and b.shape == r.shape == g.shape and float((b > 0).mean()) > 0.7
            worst[first, last] = max(worst.get((first, last), 0.0), mc.bound_ratio(g, r, b))
    print('torch fp32 against float64, max err / bound: ' + ', '.join(f'{a}-{b} {r:.2g}' for (a, b), r in worst.items()))
    assert max(worst.values()) < 1.0
    # the fp16 x2 bound contains the fp32 one
    x = mc.span_reference(sd, 0, 8, crops).astype(np.float32)
    assert (mc.span_bound(sd, 9, 9, x, 'f16x2') > mc.span_bound(sd, 9, 9, x, 'fp32')).all()


def test_f16_rtz_restatement():
    import torch
    x = np.array([0.0, 1.0, -1.0, 1.0 + 2.0 ** -10, 1.0 + 2.0 ** -11, 3.0 * 2.0 ** -25, 2.0 ** -24, 65504.0, 1e6, -0.1, 1234.567], np.float64)
    t = torch.from_numpy(x).float()
    h = t.half().double()                                    # round to nearest; toward zero = step back where it overshot
    h = torch.where(h.abs() > t.double().abs(), torch.nextafter(h.half(), torch.zeros_like(h).half()).double(), h)
    want = torch.clamp(h, -65504.0, 65504.0).numpy()
    assert np.array_equal(mc.f16_rtz(t.double().numpy()), want)
    a, b = mc.f16_pieces(1234.567)
    assert abs(1234.567 - a - b) < 2.0 ** -21 * 1234.567 and abs(b) < 2.0 ** -10 * 1234.567


SIX = [('tap', 3, (3, 3)), ('tail', 4, (4, 4)), ('halo', 2, (2, 2)), ('kswap', 9, (9, 9)), ('nores', 16, (16, 16)), ('stempad', 0, (0, 1))]
BITE = [(k, f, s, False) for k, f, s in SIX] + [(k, f, s, True) for k, f, s in SIX] + \
       [('halo', 8, (7, 14), False), ('kswap', 16, (15, 17), False), ('tail', 4, (3, 4), False)]
# What the end-of-network tolerance (1e-4 of the largest of the 62 outputs) would have let through, had a test run the faulty launch at all:
# measured here in float64 on real crops at B = 1.  Every whole-face variant moves the outputs by 2e-3 .. 0.7 of the maximum and five of the
# six one-pixel ones by 6e-4 .. 5e-2; only the one-pixel depthwise tap (1.2e-5) stays below.  The dilution through the rest of the network
# is a factor 10 .. 100, not the several decades it would take to hide a wrong band or tail: the gap the span tests close is that the old
# tests never LOOKED at most launches (one batch size for every feature, 62 numbers behind the pool at the thresholds).
UNSEEN_AT_THE_END = {('tap', 3, True)}


@pytest.mark.parametrize('kind,feature,span,pixel', BITE, ids=lambda v: str(v))
def test_wrong_variants_are_caught_by_both_probes(kind, feature, span, pixel):
    """A wrong variant (mobilenet2_cases.VARIANTS) of one block, over the whole face or in one pixel of the faulty layer's output.
    Integer probe at B = 1: a whole-face variant makes the span's output unequal (a one-pixel one can hide behind two equal hidden
    values; the figure is printed).  Gaussian checkpoint, real crops handed on: on a single block or the stem its error exceeds the fp16 x2
    bound, the wider of the two.  On a span of several blocks the propagated bound (span_bound) grows by sum |w| per layer and is far above
    any such error -- printed, not asserted: there only the integer probe bites.  The same error is then followed to the 62 outputs in
    float64 and compared with the end-of-network tolerance."""
    from synergynet_amd import synth
    first, last = span
    v = {'kind': kind, 'feature': feature, 'pixel': pixel}
    isd = mc.reference_state(mc.make_integer_state())
    x = mc.integer_input(first, 1)
    x = mc.normalize_u8(x) if first == 0 else x
    differ = int((mc.span_reference(isd, first, last, x) != mc.span_reference(isd, first, last, x, variant=v)).sum())
    assert pixel or differ > 0
    sd = synth.make_backbone_state(1234)
    crops = synth.normalize_crops(synth.make_crops(1, seed=12))
    x = crops if first == 0 else mc.span_reference(sd, 0, first - 1, crops).astype(np.float32)
    good, wrong = mc.span_reference(sd, first, last, x), mc.span_reference(sd, first, last, x, variant=v)
    ratio = mc.bound_ratio(wrong, good, mc.span_bound(sd, first, last, x, 'f16x2'))
    end = mc.rel_max(mc.span_reference(sd, last + 1, 19, wrong)[1], mc.span_reference(sd, last + 1, 19, good)[1])
    print(f"{kind}{' (one pixel)' if pixel else ''} in features.{feature}, span {first}-{last}: integer probe {differ} elements differ; gaussian "
          f'{int((good != wrong).sum())} of {good.size} differ, err / bound {ratio:.3g}, 62 outputs {end:.3g} of the maximum')
    if first == last or first == 0:
        assert ratio > 1.0
        assert (end < mc.TOL_END) == ((kind, feature, pixel) in UNSEEN_AT_THE_END)


LOWDROP = [(f, (f, f)) for f in (2, 5, 9, 12, 16)] + [(18, (18, 19)), (4, (3, 4)), (6, (5, 6)), (7, (7, 14)), (11, (7, 14)), (14, (7, 14)),
                                                     (9, (8, 14)), (13, (8, 13)), (15, (15, 17)), (16, (15, 17)), (17, (15, 17)), (17, (17, 19)),
                                                     (18, (17, 19))]


@pytest.mark.parametrize('feature,span', LOWDROP, ids=lambda v: str(v))
def test_probe_needs_the_low_fp16_piece(feature, span):
    """The probe runs the a1 b2 / b1 a2 half of the two-piece path: with the low piece of ONE layer's block-input operand dropped
    (rtz16(x) in place of x: mobilenet2_cases 'lowdrop') the span's output is unequal -- in a single block, and in a block in the
    middle or at the end of a pair, a chain or the tail, where the 12-bit operands are project outputs of the span itself."""
    first, last = span
    isd = mc.reference_state(mc.make_integer_state())
    x = mc.integer_input(first, 1)
    good = mc.span_reference(isd, first, last, x)
    wrong = mc.span_reference(isd, first, last, x, variant={'kind': 'lowdrop', 'feature': feature})
    good, wrong = (good[1], wrong[1]) if last == 19 else (good, wrong)
    differ = int((good != wrong).sum())
    print(f'low piece of the input of features.{feature} dropped, span {first}-{last}: {differ} of {good.size} elements differ')
    assert differ > 0


def test_schedule_table():
    """expected_tags against launches read off the launchers by hand, and the batch lists: every launch code is reached, and for every
    threshold t both t - 1 and t are probed."""
    full = lambda B, **k: mc.expected_tags(0, 19, B, **k)
    assert full(3) == [1, 2, 3, 4, 506, 714, 15, 16, 17, 19]
    assert full(200) == [1, 2, 3, 4, 506, 714, 15, 16, 17, 19]
    assert full(300) == [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 19]
    assert full(513) == [1, 2, 304, 506, 714, 15, 16, 17, 19]
    assert full(1024) == [1, 2, 304, 506, 714, 1517, 19] and full(1025) == [1, 2, 3, 4, 506, 714, 1517, 19]
    assert full(3, early_rm=0) == [1, 2, 3, 4, 506] + list(range(7, 18)) + [19] and full(257, early_rm=0) == [1] + list(range(2, 18)) + [19]
    assert full(3, fusion=1) == [1] + list(range(2, 18)) + [19]
    assert full(3, fusion=0) == [0, 1, 1] + [f for f in range(2, 18) for _ in range(3)] + [18, 19]
    assert mc.expected_tags(7, 13, 3) == list(range(7, 14)) and mc.expected_tags(8, 14, 3) == list(range(8, 15))       # a chain the span cuts
    assert mc.expected_tags(3, 3, 513) == [3] and mc.expected_tags(15, 16, 600) == [15, 16] and mc.expected_tags(17, 18, 3) == [17, 18]
    assert mc.expected_tags(7, 14, 384, lb_chain=2) == [7, 814] and mc.expected_tags(8, 14, 3, small_f7=0) == [814]
    assert mc.expected_tags(8, 14, 384, lb_chain=1) == [813, 14] and mc.expected_tags(8, 13, 385, lb_chain=1) == [813]
    assert mc.expected_tags(8, 14, 300, lb_chain=2, small_f7=0) == list(range(8, 15)) and mc.expected_tags(7, 14, 3, lb_chain=0) == list(range(7, 15))
    assert mc.expected_tags(0, 1, 3) == [1] and mc.expected_tags(18, 19, 3) == [19] and mc.expected_tags(17, 19, 300) == [17, 19]
    seen = set()
    for first, last in PROBED:
        for u8 in ((True, False) if first == 0 else (True,)):
            key = mc.span_key(first, last, u8)
            bs = mc.probe_batches(key)
            assert 1 in bs and bs == sorted(set(bs)) and any(b % 2 for b in bs[1:])
            assert all(b % 2 and b in bs for b in mc.ODD[key]) and mc.ODD[key]
            for t in mc.THRESHOLDS[key]:
                assert t - 1 in bs and t in bs, (key, t)
            for B in bs:
                tags = mc.expected_tags(first, last, B)
                seen |= set(tags)
                assert len(tags) <= sum(len(mc.feature_layers(f)) for f in range(first, min(last, 18) + 1)) + (last == 19)
            # both sides of every change of the launch codes themselves
            changes = [B for B in range(2, 1100) if mc.expected_tags(first, last, B) != mc.expected_tags(first, last, B - 1)]
            for t in changes:
                assert t - 1 in bs and t in bs, (key, t)
    assert seen == {1, 19, 304, 506, 714, 1517} | set(range(2, 18))
    # the slice counts of fused_block_lb4.hip's hidden-sliced schedule, restated: the batches at which the count changes
    slices = lambda B: next((d for d in (2, 3, 5, 6, 10, 15, 30) if (B + 3) // 4 * d >= 192), 30)
    assert [B for B in range(2, mc.LB4_MIN) if slices(B) != slices(B - 1)] == mc.LB4_SLICES
    assert mc.BIG in mc.probe_batches(2) and mc.BIG > 256 * 4 * 2
    for sched in ('fused-fp32', 'per-layer'):
        assert mc.probe_batches(5, sched) == [1, 3, 33]
    assert set(mc.SCHEDULES) == {'default', 'tiled', 'fused-fp32', 'per-layer'}
