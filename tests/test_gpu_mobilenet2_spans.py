"""The MobileNetV2 launches one span at a time (syn_mobilenet2_span: run_backbone itself, entered at .features[first] and left at
.features[last], on activations the test supplies), every element judged, at every batch size where the forward changes its launch.
tests/test_gpu_parity.py looks at one batch size per feature and at the 62 parameters behind the pool elsewhere; here
  * an integer probe (mobilenet2_cases.make_integer_state / integer_faces: every partial sum of every layer is an fp32 number in any order
    and every operand fits its fp16 pieces, two channels of every block input NEEDING both -- conditions asserted on the CPU in
    tests/test_mobilenet2_cpu.py) has to come out EQUAL to
    the float64 reference, and the launch codes the call returns have to be the ones mobilenet2_cases.expected_tags reads off the launchers;
  * the gaussian checkpoint has to stay within the elementwise bound of mobilenet2_cases.span_bound;
  * the spans chained in the forward's own partition equal the production forward bit for bit, and the hook refuses what it cannot run.
A batch is eight distinct faces, slot i holding face (5 i + 3) % 8; references are computed for the eight faces once and gathered on the device."""
import ctypes
import os

import numpy as np
import pytest

import mobilenet2_cases as mc

pytestmark = pytest.mark.gpu
PAD = 1024                                       # floats of NaN sentinel before and after every output region
SINGLE = [(f, f) for f in range(2, 18)]
CASES = [(0, 1, True), (0, 1, False)] + [(a, b, True) for a, b in SINGLE + mc.SPANS]
CASE_IDS = [f"{a}-{b}{'' if u8 else '-fp32crops'}" for a, b, u8 in CASES]
SCHEDS = list(mc.SCHEDULES)


@pytest.fixture(scope='module')
def handles(pack):
    """(schedule, 'integer' | 'gaussian') -> (model, state_dict), built on first use; the schedule variables are read at syn_create"""
    import torch
    assert torch.cuda.is_available()
    from synergynet_amd import synth
    from synergynet_amd.synergy3DMM import SynergyNet
    made = {}

    def get(sched, kind):
        if (sched, kind) not in made:
            fusion, early_rm = mc.SCHEDULES[sched]
            sd = mc.make_integer_state() if kind == 'integer' else synth.make_backbone_state(1234)
            os.environ['SYNERGY_HIP_FUSION'] = str(fusion)
            if sched == 'tiled':
                os.environ['SYNERGY_HIP_EARLY_RM'] = str(early_rm)
            try:
                m = SynergyNet(device='cuda:0', pack=pack, backbone_state=sd)
            finally:
                os.environ.pop('SYNERGY_HIP_FUSION', None)
                os.environ.pop('SYNERGY_HIP_EARLY_RM', None)
            assert m.numerics_report()[0] == 0, m.numerics_report()[1]        # no block fell back: the probes judge the kernels they name
            made[sched, kind] = (m, sd)
        return made[sched, kind]
    return get


def call_span(m, first, last, x, want_aux=False):
    """Runs one span through the hook into NaN-filled buffers with NaN sentinels on both sides; asserts the sentinels untouched and the
    regions free of NaN.  x: device tensor in the span's input layout (uint8 -> in_u8).  Returns (out, aux | None, launch codes)."""
    import torch
    from synergynet_amd import abi
    x = x.contiguous()
    B = x.shape[0]
    n_in, out_shape, aux_shape = mc.span_counts(first, last, B)
    assert x.numel() == n_in and x.dtype in (torch.uint8, torch.float32) and x.is_cuda
    bufs = []
    for shape in (out_shape, aux_shape if want_aux else None):
        bufs.append(None if shape is None else torch.full((2 * PAD + int(np.prod(shape)),), float('nan'), dtype=torch.float32, device=m.device))
    out, aux = bufs
    region = lambda b: b[PAD:b.numel() - PAD]
    tags = (ctypes.c_int * 64)()
    n = m._lib.syn_mobilenet2_span(m._h, first, last, x.data_ptr(), int(x.dtype == torch.uint8), B, n_in, region(out).data_ptr(), region(out).numel(),
                                   region(aux).data_ptr() if aux is not None else None, region(aux).numel() if aux is not None else 0, tags, 64,
                                   m._stream())
    if n < 0:
        abi.check(n)
    torch.cuda.synchronize()
    what = f'features {first}-{last} B={B}'
    for name, b in (('out', out), ('aux', aux)):
        if b is None:
            continue
        assert bool(torch.isnan(b[:PAD]).all()) and bool(torch.isnan(b[-PAD:]).all()), f'{what}: {name} sentinel overwritten'
        assert not bool(torch.isnan(region(b)).any()), f'{what}: {name} not fully written'
    return region(out).view(out_shape), (region(aux).view(aux_shape) if aux is not None else None), list(tags[:n])


def _first_difference(got, want):
    bad = (got != want).nonzero()
    i = tuple(int(v) for v in bad[0])
    return f'{len(bad)} of {got.numel()} elements differ, first at {i}: got {float(got[i])!r}, want {float(want[i])!r}'


def _assert_equal(got, want, what):
    import torch
    assert got.shape == want.shape, what
    assert torch.equal(got, want), f'{what}: {_first_difference(got, want)}'


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _index(B):
    import torch
    return torch.from_numpy(mc.batch_index(B)).cuda()


def _integer_probe(first, last, u8):
    """(device faces in the span's input layout, float64 reference of the eight faces cast to fp32 on the device: out | (pool, param))"""
    import torch

    def make():
        faces = mc.integer_faces(first)
        x = mc.normalize_u8(faces) if first == 0 else faces
        ref = mc.span_reference(mc.reference_state(mc.make_integer_state()), first, last, x)
        refs = tuple(torch.from_numpy(r.astype(np.float32)).cuda() for r in (ref if last == 19 else (ref,)))
        return torch.from_numpy(faces if (u8 or first) else x).cuda(), refs
    return _cached(('int', first, last, u8), make)


@pytest.mark.parametrize('first,last,u8', CASES, ids=CASE_IDS)
@pytest.mark.parametrize('sched', SCHEDS)
def test_integer_probe_matches_bit_for_bit(handles, sched, first, last, u8):
    """Every single block 2..17, the stem + features.1 from uint8 and from fp32 crops, the pairs 3-4 and 5-6, the chains 7-14 / 8-14 / 8-13,
    15-17, and the tails 17-19 / 18-19 (param and pool), at every batch of mobilenet2_cases.probe_batches: torch.equal with the float64
    reference cast to fp32, and the returned launch codes equal to expected_tags.  (8-14 and 8-13 run block by block under the default
    test knobs: the chain launches that start at features.8 belong to SYNERGY_HIP_TEST_KNOBS and are not selected by the forward.)"""
    m, _ = handles(sched, 'integer')
    fusion, early_rm = mc.SCHEDULES[sched]
    faces, refs = _integer_probe(first, last, u8)
    for B in mc.probe_batches(mc.span_key(first, last, u8), sched):
        idx = _index(B)
        out, aux, tags = call_span(m, first, last, faces[idx], want_aux=last == 19)
        what = f'{sched} features {first}-{last} B={B} launches {tags}'
        assert tags == mc.expected_tags(first, last, B, fusion, early_rm), what
        if last == 19:
            _assert_equal(aux, refs[0][idx], what + ' pool')
            _assert_equal(out, refs[1][idx], what + ' param')
        else:
            _assert_equal(out, refs[0][idx], what)


# The chain launches that START at features.8 are selected by test knobs only, and SYNERGY_HIP_TEST_KNOBS is read once per process: a child
# runs the same probe (this module's helpers) under the knobs and prints the launch codes per batch; a mismatch is its non-zero exit.
KNOB_CHILD = r'''
import json, sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import torch
import mobilenet2_cases as mc
import test_gpu_mobilenet2_spans as t
from synergynet_amd import synth
from synergynet_amd.synergy3DMM import SynergyNet
first, last, batches = int(sys.argv[3]), int(sys.argv[4]), [int(b) for b in sys.argv[5].split(',')]
m = SynergyNet(device='cuda:0', pack=synth.make_3dmm(n_vert=640), backbone_state=mc.make_integer_state())
assert m.numerics_report()[0] == 0
faces, refs = t._integer_probe(first, last, True)
tags = {}
for B in batches:
    idx = t._index(B)
    out, _, tags[B] = t.call_span(m, first, last, faces[idx])
    t._assert_equal(out, refs[0][idx], f'features {first}-{last} B={B} launches {tags[B]}')
print('TAGS ' + json.dumps(tags))
'''


@pytest.mark.parametrize('knobs,first,last,batches', [({'lb_chain': 2, 'small_f7': 0}, 8, 14, [1, 3, 256, 384, 385]),
                                                      ({'lb_chain': 1}, 8, 13, [384, 385])], ids=['8-14', '8-13'])
def test_integer_probe_on_the_chains_from_features_8(knobs, first, last, batches):
    """lb_chain = 2 / small_f7 = 0: features.8-14 in one launch (the four-stream kernel up to 256 faces, the two-face kernel from 384);
    lb_chain = 1: features.8-13.  Bit for bit on the integer probe, with the launch codes the knobs imply."""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    env = dict(os.environ, SYNERGY_HIP_TEST_KNOBS=','.join(f'{k}={v}' for k, v in knobs.items()))
    r = subprocess.run([sys.executable, '-c', KNOB_CHILD, ROOT, os.path.join(ROOT, 'tests'), str(first), str(last), ','.join(map(str, batches))],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    tags = json.loads([l for l in r.stdout.splitlines() if l.startswith('TAGS ')][-1][5:])
    for B in batches:
        assert tags[str(B)] == mc.expected_tags(first, last, B, **knobs) == [100 * first + last], (B, tags[str(B)])


def _gaussian_inputs(sd, first):
    """[(name, fp32 faces as the reference takes them, device tensor as the hook takes them)]: the fp32 cast of the float64 reference's
    previous activation on real crops (first = 0: the uint8 crops themselves), and a sign-mixed gaussian tensor scaled to the block
    input's bound of the range analysis (first = 0: fp32 crops)"""
    import torch
    from synergynet_amd import synth

    def make():
        crops = synth.make_crops(mc.N_FACES, seed=907)
        x0 = mc.normalize_u8(crops)
        chain = x0 if first == 0 else mc.span_reference(sd, 0, first - 1, x0).astype(np.float32)
        gauss = mc.gaussian_faces(first, float(mc.range_verdict(sd)[2][first]))
        assert (gauss < 0).any() and (gauss > 0).any()
        return [('chain', chain, torch.from_numpy(crops if first == 0 else chain).cuda()), ('gauss', gauss, torch.from_numpy(gauss).cuda())]
    return _cached(('gin', first), make)


def _gaussian_reference(sd, first, last, name, x, schedule):
    import torch

    def make():
        ref, bound = mc.span_reference(sd, first, last, x), mc.span_bound(sd, first, last, x, schedule)
        return (tuple(torch.from_numpy(np.ascontiguousarray(r)).cuda() for r in (ref if last == 19 else (ref,))),
                torch.from_numpy(np.ascontiguousarray(bound[0] if last == 19 else bound)).cuda())
    return _cached(('gref', first, last, name, schedule), make)


def _ratio(got, ref, bound):
    """max |got - ref| / bound on the device, float64; an element whose bound is 0 has to match exactly"""
    import torch
    err = (got.double() - ref).abs()
    assert err.shape == bound.shape
    r = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))
    return float(r.max())


@pytest.mark.parametrize('first,last,u8', [c for c in CASES if c[2]], ids=[i for i, c in zip(CASE_IDS, CASES) if c[2]])
@pytest.mark.parametrize('sched', SCHEDS)
def test_gaussian_checkpoint_within_the_bound(handles, sched, first, last, u8):
    """The ordinary checkpoint, every block and span at the first and last batch of its list, on two inputs (_gaussian_inputs):
    |got - ref64| <= span_bound elementwise -- the fp32 bound (n + 8) u (|s| sum |a||w| + |beta| + |mean s|) per layer on the fp32
    schedules, with the split terms of DESIGN 5.3 / 5.3a on the fp16 x2 schedules, propagated through sum |w| bound_in inside a span.
    With last = 19 the pool is judged by the propagated bound and the 62 outputs against a float64 head on the RETURNED pool.
    Measured on an MI355X: DESIGN 5.20.  No other tolerance."""
    m, sd = handles(sched, 'gaussian')
    schedule = 'f16x2' if mc.SCHEDULES[sched][0] >= 2 else 'fp32'
    batches = mc.probe_batches(mc.span_key(first, last, u8), sched)
    worst = {}
    for name, x, xd in _gaussian_inputs(sd, first):
        refs, bound = _gaussian_reference(sd, first, last, name, x, schedule)
        for B in (batches[0], batches[-1]):
            idx = _index(B)
            out, aux, tags = call_span(m, first, last, xd[idx], want_aux=last == 19)
            if last == 19:
                r = _ratio(aux, refs[0][idx], bound[idx])
                pool = aux.cpu().numpy()
                worst['heads', name, B] = mc.bound_ratio(out.cpu().numpy(), mc.heads_reference(sd, pool), mc.heads_bound(sd, pool))
            else:
                r = _ratio(out, refs[0][idx], bound[idx])
            worst[name, B, tuple(tags)] = r
    print(f'{sched} features {first}-{last} max(err / bound): ' + ', '.join(f'{k} {r:.3g}' for k, r in worst.items()))
    bad = {k: r for k, r in worst.items() if not r < 1.0}
    assert not bad, f'{sched} features {first}-{last}: err / bound {bad}'


def _partition(tags):
    """the spans of the forward's own launches, from the codes of a first = 0, last = 19 call"""
    spans, seen = [], []
    for t in tags:
        if seen and seen[-1] == t:                               # per-layer schedule: one code per layer
            continue
        seen.append(t)
    assert seen[-1] == 19
    for t in seen[:-1]:
        if t == 0:
            continue
        spans.append((0, 1) if t == 1 else (t // 100, t % 100) if t >= 100 else (t, t))
    if spans[-1] in ((17, 17), (18, 18)):                        # features.17 deferred to the tail / features.18 of the per-layer schedule
        spans[-1] = (spans[-1][0], 19)
    else:
        spans.append((18, 19))
    return spans


@pytest.mark.parametrize('sched,B', [('default', 3), ('default', 200), ('default', 513), ('tiled', 3), ('fused-fp32', 3), ('per-layer', 3)])
def test_chained_spans_equal_the_production_forward(handles, sched, B):
    """The spans of the forward's own partition (taken from the launch codes of a first = 0, last = 19 call), each output fed to the
    next, against forward_crops_u8 on the same handle and against the single 0..19 call: torch.equal, param and pool.  The hook runs the
    forward's launches and the forward's bits did not move."""
    import torch
    from synergynet_amd import synth
    m, _ = handles(sched, 'gaussian')
    crops = torch.from_numpy(synth.make_crops(mc.N_FACES, seed=933)).cuda()[_index(B)].contiguous()
    want, want_pool = m.forward_crops_u8(crops, return_pool=True)
    whole, whole_pool, tags = call_span(m, 0, 19, crops, want_aux=True)
    assert tags == mc.expected_tags(0, 19, B, *mc.SCHEDULES[sched]), tags
    assert torch.isfinite(want).all() and float(want.abs().max()) > 0
    assert torch.equal(whole, want) and torch.equal(whole_pool, want_pool)
    spans = _partition(tags)
    assert spans[0] == (0, 1) and spans[-1][1] == 19 and all(a[1] + 1 == b[0] for a, b in zip(spans, spans[1:])), spans
    y, issued = crops, []
    for first, last in spans[:-1]:
        y, _, t = call_span(m, first, last, y)
        issued += t
    got, got_pool, t = call_span(m, spans[-1][0], 19, y, want_aux=True)
    assert issued + t == tags, (issued + t, tags)
    assert torch.equal(got, want) and torch.equal(got_pool, want_pool)


def test_hook_refusals_leave_buffers_and_handle_alone(handles, pack):
    """Every refusal of include/synergy_hip.h: SYN_ERR_INVALID with a message that names what was expected, before any launch (the NaN
    outputs stay NaN), and the handle still passes a probe afterwards."""
    import torch
    from synergynet_amd import abi, synth
    from synergynet_amd.synergy3DMM import SynergyNet
    m, _ = handles('default', 'integer')
    lib = m._lib
    faces, refs = _integer_probe(9, 9, True)                               # features.9: [B,8,8,64] -> [B,8,8,64]
    n = 8 * 8 * 64
    xd = faces[:1].contiguous()
    out = torch.full((n + 64,), float('nan'), device='cuda')
    aux = torch.full((1280 + 64,), float('nan'), device='cuda')
    tags = (ctypes.c_int * 64)()
    other = SynergyNet(device='cuda:0', pack=pack, backbone_state=synth.make_mobilenet1_state(1357, 0.5), arch='mobilenet_05')
    crop = 3 * 120 * 120
    cases = [  # (handle, first, last, in_u8, B, n_in, n_out, aux?, n_aux, max_tags, what the message says)
        (m._h, 9, 9, 0, 1, n + 1, n, False, 0, 64, b'n_in='), (m._h, 9, 9, 0, 1, n, n - 1, False, 0, 64, b'n_out='),
        (m._h, 9, 9, 0, 1, n, n + 64, False, 0, 64, b'n_out='), (m._h, 9, 9, 0, 1, n, n, False, 1280, 64, b'n_aux='),
        (m._h, 18, 19, 0, 1, 16 * 320, 62, True, 1280 + 64, 64, b'n_aux='), (m._h, 18, 19, 0, 1, 16 * 320, 62, True, 0, 64, b'n_aux='),
        (m._h, 9, 9, 0, 2, n, n, False, 0, 64, b'B=2'),                     # counts of one face offered for two
        (other._h, 9, 9, 0, 1, n, n, False, 0, 64, b'mobilenet_05'),
        (m._h, 10, 9, 0, 1, n, n, False, 0, 64, b'first=10'), (m._h, -1, 9, 0, 1, n, n, False, 0, 64, b'first=-1'),
        (m._h, 9, 20, 0, 1, n, n, False, 0, 64, b'last=20'), (m._h, 19, 19, 0, 1, n, n, False, 0, 64, b'first=19'),
        (m._h, 1, 9, 0, 1, n, n, False, 0, 64, b'first=1'), (m._h, 0, 0, 0, 1, crop, n, False, 0, 64, b'last=0'),
        (m._h, 9, 9, 1, 1, n, n, False, 0, 64, b'in_u8'), (m._h, 9, 9, 0, 1, n, n, True, 1280, 64, b'aux'),
        (m._h, 9, 9, 0, 0, 0, 0, False, 0, 64, b'B=0'), (m._h, 9, 9, 0, -1, n, n, False, 0, 64, b'B=-1'), (m._h, 9, 9, 0, 65537, n, n, False, 0, 64, b'B=65537'),
        (m._h, 9, 9, 0, 1, n, n, False, 0, 2, b'max_tags=2'), (m._h, 18, 19, 0, 1, 16 * 320, 62, False, 0, 1, b'max_tags=1'),
        (m._h, 9, 9, 0, 1, n, n, False, 0, -1, b'max_tags=-1'),
    ]
    for h, first, last, u8, B, ni, no, with_aux, na, mt, word in cases:
        rc = lib.syn_mobilenet2_span(h, first, last, xd.data_ptr(), u8, B, ni, out.data_ptr(), no, aux.data_ptr() if with_aux else None, na, tags, mt,
                                     m._stream())
        err = lib.syn_last_error()
        assert rc == abi.SYN_ERR_INVALID, (first, last, u8, B, ni, no, with_aux, na, mt)
        assert b'syn_mobilenet2_span' in err and b'expected' in err and word in err, err
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(aux).all())
    got, _, t = call_span(m, 9, 9, xd)
    assert t == [9]
    _assert_equal(got, refs[0][:1], 'after the refusals')
